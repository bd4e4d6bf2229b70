"""Every instantiation of the one-pass family table (k_fused_compact<XR = 2, ..., FAM>, bz_families.inc) against the
oracle, in fp64 and fp32.  A family is (f kind, g kind, D class) with c = Identity; its code is
fam_code(fk, gk, dk) = fk | gk << 1 | dk << 4 (bz_kernels.h), and each code has its own parameter streams (g's u, g's
and D's vector bounds, mu and mu*y unless uniform / zero) and pipeline depth.  So each of the 96 families per type is
its own code path, and this file runs every one of them:
  (a) 30 PANOCplus states against the oracle, once with per-element penalties (UNI = 0) and once with uniform ones
      (UNI = 1, or UNI = 2 with zero multipliers), the default-policy and the non-temporal instantiation (NT = 0 / 1)
      both taken; the compile-time UNI is the host's own choice, confirmed from the form string;
  (b) the compile-time instantiation, the run-time one (BZ_FAMRT=1) and the stored-pair form (BZ_XR=0) bit for bit on
      one pinned grid, from a start far enough out that tau-backtracked passes go through the TRIAL instantiation.
The families whose subproblem has no smooth part (DEGENERATE) are run against the oracle for what they do instead.
Sizes leave the last pack ragged (fp64 packs hold 2 elements, fp32 packs 4), and the pinned grid of (b) is wider than
every n here, so most of its threads start past the last full pack."""
import zlib

import numpy as np
import pytest

from tests.test_gpu_families import SCALARS
from tests.test_gpu_parity import RTOL_ITER, iter_tol, run_traces

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# the kinds of bz_kernels.h (FAM_F_*, FAM_G_*, FAM_D_*); test_host_logic checks these against the header
FAM_F = {"zero": 0, "diag": 1}
FAM_G = {"zero": 0, "l1": 1, "nonneg": 2, "l1box": 3, "indbox": 4, "indbox_vec": 5}
FAM_D = {"zero": 0, "free": 1, "box": 2, "box_vec": 3, "vc": 4, "cc": 5, "eitheror": 6, "xor": 7}
PAIRWISE = ("vc", "cc", "eitheror", "xor")


def fam_code(fk, gk, dk):
    return fk | (gk << 1) | (dk << 4)


# IndBox g with vector bounds and Box D with vector bounds: both sides vectors, or one side a vector and the other a
# scalar (an infinite one, or a finite one) — rotated over the families of the class
G_VEC_FORMS = ("both", "lo_vec_hi_inf", "lo_num_hi_vec")
D_VEC_FORMS = ("both", "lo_vec_hi_inf", "lo_num_hi_vec")

FAMILIES = [(f, g, D) for f in FAM_F for g in FAM_G for D in FAM_D]
assert len(FAMILIES) == 96

# f = Zero with D = Free: the augmented Lagrangian of the subproblem is identically zero (no f, and c(x) + mu*y is
# always in D), so the smoothness estimate is 0 and gamma = alpha / 0 — there is no iteration to compare, only what
# both sides do with it
DEGENERATE = {("zero", g, "free"): "f = Zero and D = Free: the smooth part is identically 0, L = 0, gamma = alpha / 0"
              for g in FAM_G}


def fid(fam):
    return "-".join(fam)


def variant(fam):
    """the vector-bound form of a family's IndBox g / Box D (rotated over the families, so every form is run)"""
    f, g, D = fam
    i = FAM_F[f] * 8 + FAM_D[D] + FAM_G[g]
    return G_VEC_FORMS[i % 3], D_VEC_FORMS[i % 3]


def expected_code(fam):
    f, g, D = fam
    return fam_code(FAM_F[f], FAM_G[g], FAM_D[D])


def make_case(bz, ref, n, fam, dtype, regime, far=False):
    """(device oracles, reference oracles, mu, y, x0) for family `fam` in type `dtype`.
    regime: "uni0" per-element mu and y != 0; "uni1" uniform mu, y != 0; "uni2" uniform mu, y = 0.
    far: a start far from the solution (larger multipliers, a large x0): tau backtracks happen."""
    f, g, D = fam
    T = np.dtype(dtype).type
    gform, dform = variant(fam)
    d = bz.synth.l1_quadratic(n, dtype=dtype)
    rng = np.random.default_rng(zlib.crc32(("%s-%s-%s" % (fid(fam), np.dtype(dtype).name, regime)).encode()))
    scale = 0.2 if D in PAIRWISE else 1.0
    r = np.random.default_rng(zlib.crc32(fid(fam).encode()) + 1)
    u = np.where(np.arange(n) % 5 == 0, 0.0, r.uniform(0.3, 1.0, n)).astype(dtype)
    glo, ghi = (-r.uniform(0.2, 1.0, n)).astype(dtype), r.uniform(0.2, 1.0, n).astype(dtype)
    dlo, dhi = (-r.uniform(0.1, 1.0, n)).astype(dtype), r.uniform(0.1, 1.0, n).astype(dtype)
    out = []
    for m in (bz, ref):
        # (scalar parameters: numbers of the type for the oracle, Python floats for the device)
        num = (lambda v: T(v)) if m is ref else float
        ff = m.DiagQuadratic(d["q"], (scale * d["b"]).astype(dtype)) if f == "diag" else m.Zero()
        if g == "l1":
            gg = m.NormL1(num(0.8))
        elif g == "nonneg":
            gg = m.NormL1Nonneg(num(0.8))
        elif g == "l1box":
            gg = m.NormL1Box(num(0.8), u=u)
        elif g == "indbox":
            gg = m.IndBox(num(-0.5), num(0.5))
        elif g == "indbox_vec":
            gg = {"both": lambda: m.IndBox(glo, ghi), "lo_vec_hi_inf": lambda: m.IndBox(glo, num(np.inf)),
                  "lo_num_hi_vec": lambda: m.IndBox(num(-0.4), ghi)}[gform]()
        else:
            gg = m.Zero()
        if D == "box":
            DD = m.ClosedSet(m.IndBox(num(-1.0), num(1.0)))
        elif D == "box_vec":
            DD = m.ClosedSet({"both": lambda: m.IndBox(dlo, dhi), "lo_vec_hi_inf": lambda: m.IndBox(dlo, num(np.inf)),
                              "lo_num_hi_vec": lambda: m.IndBox(num(-0.6), dhi)}[dform]())
        elif D == "free":
            DD = m.FreeSet()
        elif D == "zero":
            DD = m.ZeroSet()
        else:
            DD = m.PairwiseSet(D)
        out.append((ff, gg, m.IdentityFunction(), DD))
    if regime == "uni0":
        mu = (10.0 ** rng.uniform(-2, 0, n)).astype(dtype)
    else:
        mu = np.full(n, 0.1, dtype)
    # (f = Zero: multipliers large enough that c(x) + mu*y leaves D — otherwise the subproblem is min g(x), solved at 0
    # in two iterations; with y = 0 the start is put outside D instead)
    ys = (30.0 if f == "zero" else 1.0) * (5.0 if far else 1.0)
    y = np.zeros(n, dtype) if regime == "uni2" else (ys * rng.standard_normal(n)).astype(dtype)
    # (far with D = Free: a unit start — from three units out those classes converge without a tau backtrack)
    xs = (1.0 if D == "free" else 3.0) if far else (3.0 if f == "zero" and regime == "uni2" else 0.3)
    x0 = (xs * rng.standard_normal(n)).astype(dtype)
    return out[0], out[1], mu, y, x0


def oracle_size(fam, dtype, i):
    """low thousands; fp64: odd (pairwise sets: n = 2 mod 4), fp32: n % 4 in {1, 2, 3} (pairwise sets: 2)"""
    base = 2000 + 40 * (i % 7)
    if np.dtype(dtype).itemsize == 8:
        return base + (2 if fam[2] in PAIRWISE else 1)
    return base + (2 if fam[2] in PAIRWISE else (1, 2, 3)[i % 3])


def oracle_regimes(fam, i):
    """(regime, NT) pairs of a family: per-element penalties, and a uniform regime rotated over the families (f = Zero
    never takes y = 0: see make_case); NT = 1 for one of the two, alternating, so every family runs both halves of
    the table"""
    other = "uni1" if (fam[0] == "zero" or i % 2 == 0) else "uni2"
    return [("uni0", i % 2 == 1), (other, i % 2 == 0)]


def bitwise_size(fam, dtype, i):
    """the sizes of the bitwise sweep: ragged as in oracle_size, and every fourth family tiny (a hundred elements on a
    grid of 512 x 256 threads: nearly every thread clamps)"""
    base = 100 if i % 4 == 0 else 20_000
    if fam[2] in PAIRWISE:
        return base + 2
    return base + (1 if np.dtype(dtype).itemsize == 8 else (1, 2, 3)[i % 3])


# one case per (family, type, penalty regime): the regimes of oracle_regimes, each with its own NT
ORACLE_CASES = [(fam, dt, r) for dt in ("float64", "float32") for fam in FAMILIES if fam not in DEGENERATE
                for r in (0, 1)]
# Open finding (NEXT.md), present before this file: f = Zero, g = L1Box, D = Zero, uniform penalties, fp64 — the device's
# residual decays to ~1e-180 where the oracle's is exactly 0, the curvature <s, y> of the last pairs becomes subnormal,
# and at k = 20 the compact L-BFGS form turns x into NaN.  Only this (family, type, regime) case is a strict xfail.
NAN_AFTER_CONVERGENCE = [(("zero", "l1box", "zero"), "float64", 1)]
# f = Zero with the L1Box g: the first iterations are tau backtracks on both sides (up to 300 in 30 iterations), so
# fewer of them are one-pass iterations
FEW_ONE_PASS = {("zero", "l1box", D) for D in FAM_D}


# The headline family's plain passes take the specialised headline kernel (test_gpu_lds_ring, test_gpu_param_residency);
# its table entry is reached through BZ_FAMRT=1, in the run-time UNI / TRIAL instantiation.  (Its compile-time UNI
# entries serve BZ_SPEC=0 only.)
HEADLINE = ("diag", "l1", "box")


def _forms(fam, regime, nt, famrt=False):
    """(plain pass, tau-backtracked pass) forms of a family's table instantiations"""
    code = expected_code(fam)
    trial = "k_fused_compact<XR=2,UNI=-1,NT=%d,TRIAL=-1,FAM=%d>" % (nt, code)
    if famrt:
        return trial, trial
    return "k_fused_compact<XR=2,UNI=%s,NT=%d,TRIAL=0,FAM=%d>" % (regime[-1], nt, code), trial


def _traces(bz, ref, monkeypatch, fam, dtype, n, regime, nt, iters=30):
    dev, orc, mu, y, x0 = make_case(bz, ref, n, fam, dtype, regime)
    if nt:
        monkeypatch.setenv("BZ_NT", "1")
    else:
        monkeypatch.delenv("BZ_NT", raising=False)
    if fam == HEADLINE:
        monkeypatch.setenv("BZ_FAMRT", "1")
    forms = []
    with np.errstate(all="ignore"):
        prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, iters, dtype=dtype,
                                    minimum_gamma=float(np.finfo(dtype).eps), forms=forms)
    prob.close()
    return rows, forms


@pytest.mark.parametrize("fam,dt,r", [pytest.param(*c, marks=pytest.mark.xfail(
    strict=True, reason="subnormal L-BFGS curvature after convergence: x turns NaN on the device only (NEXT.md)"))
    if c in NAN_AFTER_CONVERGENCE else c for c in ORACLE_CASES],
                         ids=["%s-%s-%d" % (fid(f), d[-2:], r) for f, d, r in ORACLE_CASES])
def test_family_instantiation_follows_oracle(bz, ref, monkeypatch, fam, dt, r):
    for k in ("BZ_XR", "BZ_UNI", "BZ_GFC", "BZ_GRID", "BZ_TRIALFUSE", "BZ_FAMRT", "BZ_NT", "BZ_SKIPZ"):
        monkeypatch.delenv(k, raising=False)
    dtype = np.dtype(dt).type
    i = FAMILIES.index(fam)
    n = oracle_size(fam, dtype, i)
    fp64 = dtype == np.float64
    regime, nt = oracle_regimes(fam, i)[r]
    rows, forms = _traces(bz, ref, monkeypatch, fam, dtype, n, regime, nt)
    # the plain pass ran in this family's compile-time instantiation with the UNI the host chose; any other form
    # seen is the same family's TRIAL (run-time UNI / TRIAL) instantiation of a tau-backtracked pass
    plain, trial = _forms(fam, regime, nt, famrt=fam == HEADLINE)
    assert plain in forms and set(forms) <= {plain, trial}, (regime, plain, sorted(set(forms)))
    assert sum(r_[7] for r_ in rows) >= (10 if fam in FEW_ONE_PASS else 20), (regime, [r_[7] for r_ in rows])
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        if fp64:
            assert abs(g_d - g_r) <= 1e-13 * g_r, (regime, k, g_d, g_r)
            tol = iter_tol(sens)
            assert abs(sn_d - sn_r) <= 1e-8 * max(1.0, sn_r), (regime, k, sn_d, sn_r)
        else:
            tol = max(2e-5, 100 * sens)
            # (while the oracle's own two roundings agree to 2e-7: past that, a gamma halving — an fp32 comparison
            # of f(z) with its model — is no longer decided by the restatement)
            if tol == 2e-5:
                assert abs(g_d - g_r) <= 1e-5 * g_r, (regime, k, g_d, g_r)
        assert ex <= tol and ez <= tol, f"{regime}: iterate mismatch at k={k}: {ex} {ez} (tol {tol})"
    # the widened tolerance (the oracle's own rounding sensitivity) may not carry the comparison: f = Zero families
    # collapse onto their solution within a few iterations, the others stay in a tight band for most states (fp64: the
    # north-star 1e-10; fp32: 1e-3 — the fp32 oracle's two roundings part by 1e-7..1e-6 within a few states, and by more
    # than 1e-5 after 10 to 19 states in the roughest cases)
    tight = sum(1 for r_ in rows if (iter_tol(r_[8]) == RTOL_ITER if fp64 else max(2e-5, 100 * r_[8]) <= 1e-3))
    assert tight >= ((5, 20) if fp64 else (2, 10))[fam[0] == "diag"], (regime, tight)


@pytest.mark.parametrize("dt", ["float64", "float32"])
@pytest.mark.parametrize("fam", sorted(DEGENERATE), ids=[fid(f) for f in sorted(DEGENERATE)])
def test_degenerate_family_does_what_the_oracle_does(bz, ref, monkeypatch, fam, dt):
    """No smooth part: gamma = alpha / 0 on both sides, and from there the same NaN / inf pattern in every state."""
    for k in ("BZ_XR", "BZ_UNI", "BZ_GFC", "BZ_GRID", "BZ_TRIALFUSE", "BZ_FAMRT", "BZ_NT", "BZ_SKIPZ"):
        monkeypatch.delenv(k, raising=False)
    dtype = np.dtype(dt).type
    n = oracle_size(fam, dtype, FAMILIES.index(fam))
    dev, orc, mu, y, x0 = make_case(bz, ref, n, fam, dtype, "uni0")
    prob = bz.Problem(*dev, n, n, dtype)
    prob.set_multipliers(mu, y)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps),
                                  directions=bz.LBFGS(5)).c_opts(), x0)
    with np.errstate(all="ignore"):
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=float(np.finfo(dtype).eps))
        st = it.init()
        try:
            for k in range(4):
                sc = prob.panoc_scalars()
                xd, zd = prob.panoc_vector("x"), prob.panoc_vector("z")
                g_d, g_r = sc["gamma"], float(st.gamma)
                assert (np.isnan(g_d), np.isinf(g_d)) == (np.isnan(g_r), np.isinf(g_r)), (k, g_d, g_r)
                assert not np.isfinite(g_r), g_r        # (the case is degenerate on the oracle's side)
                for a, b in ((xd, st.x), (zd, st.z)):
                    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), k
                    fin = np.isfinite(b)
                    assert np.array_equal(a[fin], b[fin]), k
                prob.panoc_step()
                st = it.step(st)
        finally:
            prob.close()


def _lockstep(bz, dev, n, mu, y, x0, iters, envs, dtype, monkeypatch):
    """_run of test_gpu_families for several forms side by side: every state (x, z, res, the scalars, the counters and
    the form of the one-pass launch) after every step"""
    knobs = ("BZ_XR", "BZ_UNI", "BZ_GFC", "BZ_GRID", "BZ_TRIALFUSE", "BZ_FAMRT", "BZ_SKIPZ", "BZ_NT")
    eps = float(np.finfo(dtype).eps)
    probs = []
    try:
        for env in envs:
            for k in knobs:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            prob = bz.Problem(*dev, n, n, dtype)
            probs.append(prob)
            prob.set_multipliers(mu, y)
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps, directions=bz.LBFGS(5)).c_opts(), x0)
        runs = [[] for _ in envs]
        for _ in range(iters):
            states = []
            for prob in probs:
                prob.panoc_step()
                st = prob.panoc_stats()
                states.append((prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"),
                               prob.panoc_scalars(), (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips,
                                                      st.n_fused_iters), prob.profile2()["k_fused_iterates"]["form"]))
            for r, s_ in zip(runs, states):
                r.append(s_)
        return runs
    finally:
        for prob in probs:
            prob.close()


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


GD_CLASSES = [(g, D) for g in FAM_G for D in FAM_D]
# The two runs (family, type, regime) in which a step uses up its 20 trials, steps 42 to 45: the forms used to part there (a
# gamma halving in a step's last trial, NEXT.md "Line search at its limit"); tests/test_gpu_linesearch_table.py holds the
# same runs to the oracle.  Asserted below: both are among the runs of their class's test.
EXHAUSTED_BACKTRACKS = [(("diag", "l1", "cc"), "float32", "uni0"), (("zero", "indbox_vec", "box_vec"), "float64", "uni0")]
# (g, D) classes where no tau backtrack can be asked for: g = Zero, D = Free leaves a separable strongly convex quadratic
# with f = DiagQuadratic (the oracle accepts every quasi-Newton step from every start tried, n = 2e4, 60 steps) and the
# degenerate family with f = Zero
NO_TRIAL_CLASSES = {("zero", "free"): "f = DiagQuadratic: a separable quadratic, every quasi-Newton step accepted; "
                                      "f = Zero: degenerate"}


def _bitwise_runs(fam, dtype):
    """(regime, far start, NT) of the bitwise sweep: per-element penalties from a far start, and a uniform regime"""
    i = FAMILIES.index(fam)
    return [("uni0", True, False), ("uni1" if i % 2 else "uni2", False, i % 2 == 0)]


def _bitwise_run(bz, ref, monkeypatch, fam, dt, regime, far, nt, iters=60):
    """the compile-time instantiation, the run-time one and the stored-pair form of one family, type and regime, state
    by state on one pinned grid; returns whether a tau-backtracked pass went through the family's TRIAL instantiation"""
    dtype = np.dtype(dt).type
    n = bitwise_size(fam, dtype, FAMILIES.index(fam))
    dev, orc, mu, y, x0 = make_case(bz, ref, n, fam, dtype, regime, far=far)
    p = {"BZ_GFC": "2", "BZ_GRID": "512"}
    if nt:
        p["BZ_NT"] = "1"
    envs = [dict(p, BZ_XR="0", BZ_TRIALFUSE="0"), dict(p, BZ_XR="2", BZ_TRIALFUSE="1"),
            dict(p, BZ_XR="2", BZ_FAMRT="1", BZ_TRIALFUSE="1")]
    base, *others = _lockstep(bz, dev, n, mu, y, x0, iters, envs, dtype, monkeypatch)
    case = (fam, dt, regime, n)
    assert not any("FAM=" in b[5] for b in base), base[-1][5]
    trial_seen = False
    for env, r in zip(envs[1:], others):
        ct = "BZ_FAMRT" not in env
        for k, (a, b) in enumerate(zip(r, base)):
            for u, v in zip(a[:3], b[:3]):
                assert np.array_equal(u, v, equal_nan=True), (case, env, k + 1)
            # (the degenerate families: gamma = alpha / 0 — their scalars are compared with the oracle's in
            # test_degenerate_family_does_what_the_oracle_does)
            for key in SCALARS if fam not in DEGENERATE else ():
                assert _same(a[3][key], b[3][key]), (case, env, k + 1, key)
            assert a[4][:3] == b[4][:3], (case, env, k + 1, a[4], b[4])
        forms = set(a[5] for a in r if a[5])
        plain, trial = _forms(fam, regime, nt, famrt=not ct)
        if ct and fam == HEADLINE:      # (the headline kernel, against the same stored-pair base)
            assert not any("FAM=" in f_ for f_ in forms), sorted(forms)
        else:
            assert forms <= {plain, trial}, (case, env, sorted(forms))
        if fam not in DEGENERATE:      # (those may leave the one-pass form once gamma is not finite)
            assert fam == HEADLINE and ct or plain in forms, (case, env, sorted(forms))
            assert r[-1][4][3] >= 4, (case, env, r[-1][4])      # (one-pass iterations)
        if ct and trial in forms and fam not in DEGENERATE:      # (the plain form is not TRIAL=-1)
            trial_seen = True
    return trial_seen


@pytest.mark.parametrize("g,D", GD_CLASSES, ids=["%s-%s" % c for c in GD_CLASSES])
def test_family_forms_are_bitwise_neutral_over_the_table(bz, ref, monkeypatch, g, D):
    """Both f kinds and both types of one (g, D) class: the compile-time instantiation, the run-time one and the
    stored-pair form give the same bits on one pinned grid; at least one run of the class sent a tau-backtracked pass
    through the family's TRIAL instantiation."""
    trial_passes = 0
    for dt in ("float64", "float32"):
        for f in FAM_F:
            fam = (f, g, D)
            for regime, far, nt in _bitwise_runs(fam, dt):
                trial_passes += _bitwise_run(bz, ref, monkeypatch, fam, dt, regime, far, nt)
    if (g, D) not in NO_TRIAL_CLASSES:
        assert trial_passes >= 1, "no tau-backtracked pass went through a TRIAL instantiation of this (g, D) class"


def test_runs_with_exhausted_backtracks_are_runs_of_their_class():
    for fam, dt, regime in EXHAUSTED_BACKTRACKS:
        assert (regime, True) in [(r, far) for r, far, nt in _bitwise_runs(fam, dt)], (fam, dt, regime)
