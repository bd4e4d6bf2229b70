"""The outer loops of alps and als (bz_alps_solve / bz_als_solve: k_penalty_init, k_muy with the dual safeguard and the
uniform-penalty probe, k_dual_update, k_dual_update_slack, k_clamp_scale, their C++ copy for callback oracles, and the host
decisions around them — have_old, the theta test, the tolerance schedule, the buffer swap) against the oracle BIT FOR BIT,
for every g, D and type.

The subsolver is PANOCplus(maxit=1, gamma=GAMMA, adaptive=False) on both sides: one state, a fixed step, so with
c = Identity and an element-wise f every outer quantity is an element-wise function of the inputs (the library is built
with -ffp-contract=off), norm_res_prim is a maximum and the penalty denominator max(1, objx) is exactly 1 (the generator
of tests/test_outer_loop_host.py keeps the start's objective below 1; its preconditions are checked there on the oracle
alone).  The device returns only the final state, so it runs with maxit = 1 .. K and each run is compared with the
oracle's state after as many iterations.

The Lp kinds of g are left out: their prox goes through pow, which is not correctly rounded on either side."""
import warnings

import numpy as np
import pytest

from tests.test_gpu_parity import LongDoubleReducer
from tests.test_outer_loop_host import (K_OUTER, PAIRWISE, SPECIAL_N, TYPES, als_case, als_cases, class_theta, class_variant,
                                        matrix_case, matrix_cases, matrix_oracle_runs, oracle_states, pack_of,
                                        special_classes, special_outer_case, sub_factory, table_case, table_cases, theta_tie_case,
                                        uni_of)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KNOBS = ("BZ_UNI", "BZ_XR", "BZ_GFC", "BZ_GRID", "BZ_NT", "BZ_FAMRT", "BZ_FUSEDBEGIN")
ENTRIES = (0, 1, 2, 3, 5, 6, 7, 8, 9)          # of the returned 10-tuple: all but the elapsed time
NAMES = {0: "x", 1: "y", 2: "tot_it", 3: "tot_inner_it", 5: "status", 6: "inner_tol", 7: "norm_res_prim", 8: "s", 9: "mu"}
UNI_SEEN = {}          # (type, uni) -> subproblems whose bytes showed that value of P.uni


def _same_bits(a, b):
    """equal values, NaN positions compared as positions, zeros by sign"""
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)
            and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b)))


def _same_number(a, b):
    if a is None or b is None:
        return a is None and b is None
    return float(a) == float(b) or (np.isnan(a) and np.isnan(b))


def first_difference(a, b):
    bad = np.flatnonzero(~(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))          # (a NaN has no sign here)
    return [(int(i), a[i], b[i]) for i in bad[:4]], int(bad.size)


def assert_state(got, want, tag):
    """got: a returned 10-tuple; want: the oracle's (x, y, tot_it, tot_inner_it, status, inner_tol, norm_res_prim, s, mu)"""
    for e, w in zip(ENTRIES, want):
        a = got[e]
        if isinstance(w, np.ndarray):
            assert a.dtype == w.dtype and _same_bits(a, w), (tag, NAMES[e]) + first_difference(a, w)
        elif e in (6, 7):
            assert _same_number(a, w), (tag, NAMES[e], a, w)
        else:
            assert a == w, (tag, NAMES[e], a, w)


def as_state(o):
    return tuple(o[e] for e in ENTRIES)


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def d_vector_streams(D, dform):
    return 0 if D != "box_vec" else (2 if dform == "both" else 1)


# ------------------------------------------------------------------ (2) alps, every g x D x type
TABLE = table_cases()


@pytest.mark.parametrize("g,D,dt,layout", TABLE, ids=["%s-%s-%s%s" % (g, D, dt[-2:], "" if lay == "adjacent" else "-split")
                                                      for g, D, dt, lay in TABLE])
def test_alps_outer_loop_bit_for_bit(bz, ref, monkeypatch, g, D, dt, layout):
    """K = 6 outer iterations around one-state subsolves: for maxit = 1 .. 6 the resident loop and the host loop around
    the device subsolver (resident=False) return the oracle's bits in x, y, s and mu, and its tot_it, tot_inner_it,
    status, inner_tol and norm_res_prim.  The bytes of the subproblems' first pass (k_begin_lip streams mu and mu*y unless
    the probe of k_muy reported them uniform / zero) show which P.uni each subproblem ran with: it must be what the
    oracle's penalties and multipliers say."""
    _clear(monkeypatch)
    case, regime, n = table_case(g, D, dt, layout, bz=bz, ref=ref)
    theta = class_theta(g, D)
    with np.errstate(all="ignore"):
        states, entering, _ = oracle_states(ref, case, theta_penalty=theta)
    dtype = np.dtype(dt)
    f = case["key"][0]
    dform = class_variant(g, D)[1]
    prob = bz.Problem(*case["dev"], n, n, dtype)
    try:
        for k in range(1, K_OUTER + 1):
            tag = (g, D, dt, layout, regime, n, "maxit=%d" % k)
            prob.profile_reset()
            a = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=theta,
                        problem=prob)
            assert_state(a, states[k - 1], tag + ("resident",))
            p = prob.profile2()["al_gradient"]
            its = states[k - 1][2]
            # l0box has no one-pass family: the probe does not run for it, mu and mu*y are streamed
            unis = [0 if g == "l0box" else uni_of(*entering[j]) for j in range(its)]
            want = sum(2 + (2 if f == "diag" else 0) + 2 - u + d_vector_streams(D, dform) for u in unis) * n * dtype.itemsize
            assert p["launches"] == its and p["bytes"] == want, (tag, p["launches"], its, p["bytes"] / (n * dtype.itemsize),
                                                                  want / (n * dtype.itemsize), unis)
            if k == K_OUTER:
                for u in unis:
                    UNI_SEEN[(dt, u)] = UNI_SEEN.get((dt, u), 0) + 1
            b = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=theta,
                        resident=False)
            assert_state(b, states[k - 1], tag + ("host loop",))
    finally:
        prob.close()


@pytest.mark.parametrize("dt", TYPES)
def test_theta_test_is_strict_at_a_tie(bz, ref, monkeypatch, dt):
    """norm_res_prim == theta_penalty * norm_res_prim_old exactly at every decision (theta_tie_case): `>` leaves the
    penalties alone, `>=` would halve them"""
    _clear(monkeypatch)
    case = theta_tie_case(dt, bz=bz, ref=ref)
    n = case["x0"].shape[0]
    states, _, decisions = oracle_states(ref, case, theta_penalty=1.0)
    assert decisions and all(nrp == bound and not taken for _, taken, nrp, bound in decisions)
    for k in range(1, K_OUTER + 1):
        for resident in (True, False):
            a = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=1.0,
                        resident=resident)
            assert_state(a, states[k - 1], (dt, n, "maxit=%d" % k, "resident" if resident else "host loop"))


def test_zz_uniform_penalties_travelled_as_numbers():
    """reads what the table above observed (run the file whole): subproblems with P.uni = 0, 1 and 2 in both types"""
    print("subproblems per (type, P.uni):", sorted(UNI_SEEN.items()))
    assert all(UNI_SEEN.get((dt, u), 0) > 0 for dt in TYPES for u in (0, 1, 2)), UNI_SEEN


# ------------------------------------------------------------------ (3) arguments where the arithmetic branches
SPECIAL = special_classes()


@pytest.mark.parametrize("mode", ["finite", "nan_y", "nan_x"])
@pytest.mark.parametrize("g,D,dt", SPECIAL, ids=["%s-%s-%s" % (g, D, dt[-2:]) for g, D, dt in SPECIAL])
def test_outer_arguments_where_the_arithmetic_branches(bz, ref, monkeypatch, g, D, dt, mode):
    """One outer iteration (maxit = 1) from x0 and y0 that hold the values where k_penalty_init, the safeguard of k_muy and
    k_dual_update branch (special_outer_case): x, y, s and mu with the oracle's bits and NaN positions, the same counts,
    status and norm_res_prim, from the resident loop and from the host loop.
    Julia's min / max return a NaN argument, so default_dual_safeguard! leaves a NaN multiplier NaN and
    default_penalty_parameter! a NaN distance NaN; the run then ends as :exception.  With maxit = 1 the status is
    :max_iter either way (`tired` is asked first), so the runs with NaN are also made with maxit = 2, where the oracle
    stops after the first iteration (or before it)."""
    _clear(monkeypatch)
    n = SPECIAL_N[(dt, D in PAIRWISE)]
    case = special_outer_case(g, D, dt, n, mode, bz=bz, ref=ref)
    for maxit in ((1,) if mode == "finite" else (1, 2)):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = ref.alps(*case["orc"], case["x0"], case["y0"].copy(), maxit=maxit, subsolver=sub_factory(ref))
            for resident in (True, False):
                a = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=maxit, subsolver=sub_factory(bz), resident=resident)
                assert_state(a, as_state(o), (g, D, dt, mode, "maxit=%d" % maxit, "resident" if resident else "host loop"))


# ------------------------------------------------------------------ (4) als, the slack form
ALS = als_cases()


@pytest.mark.parametrize("g,D,dt", ALS, ids=["%s-%s-%s" % (g, D, dt[-2:]) for g, D, dt in ALS])
def test_als_outer_loop_bit_for_bit(bz, ref, monkeypatch, g, D, dt):
    """The same lock-step through bz.als / ref.als (slack form, c = Identity): k_penalty_init writing s into xs[nx:],
    k_dual_update_slack and the device-to-device copy of xs between two subproblems.  nx is a multiple of the pack (the
    slack form needs it) and nx / pack no multiple of the block: the grid is ragged."""
    _clear(monkeypatch)
    case, regime, n = als_case(g, D, dt, bz=bz, ref=ref)
    theta = class_theta(g, D)
    assert n % pack_of(dt) == 0 and (n == pack_of(dt) or (n // pack_of(dt)) % 256)
    for k in range(1, K_OUTER + 1):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = ref.als(*case["orc"], case["x0"], case["y0"].copy(), maxit=k, subsolver=sub_factory(ref), theta_penalty=theta)
        for resident in (True, False):
            a = bz.als(*case["dev"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=theta,
                       resident=resident)
            assert_state(a, as_state(o), (g, D, dt, regime, n, "maxit=%d" % k, "resident" if resident else "host loop"))


# ------------------------------------------------------------------ (5) beside a matrix: sums have an order
MATRIX = matrix_cases()
MATRIX_WORST = {}          # (kind, type, quantity) -> (device distance / scale, sens / scale): printed by the tally below


@pytest.mark.parametrize("kind,shape,D,dt", MATRIX, ids=["%s-%dx%d-%s-%s" % (k, s[0], s[1], D, dt[-2:]) for k, s, D, dt in MATRIX])
def test_outer_loop_beside_a_matrix(bz, ref, monkeypatch, kind, shape, D, dt):
    """c(x) = A x - b (DenseAffine and SparseAffine under alps — one CSR matrix with cut rows —, DenseAffine under als:
    k_dual_update_slack_rows), and f = SparseLeastSquares beside c = Identity from an objective above 1 (the penalty
    denominator is a reduced value there), maxit = 1 .. 4.  The counts, the status, inner_tol and every penalty decision
    (a flipped one changes mu by a factor 2; tests/test_outer_loop_host.py shows that every decision has a margin) are the
    oracle's.  x, y, s, mu and norm_res_prim are within max(base * scale, 100 * sens): base = 1e-12 (fp64) / 2e-5 (fp32) of
    the quantity's largest entry, the bound for order-dependent sums of test_general_gradient_against_oracle_and_dense_kind;
    sens = the distance between the oracle and its twin whose sums are carried in extended precision."""
    _clear(monkeypatch)
    case = matrix_case(kind, shape, D, dt, bz=bz, ref=ref)
    runs = matrix_oracle_runs(ref, case)
    twins = matrix_oracle_runs(ref, case, LongDoubleReducer())
    base = 1e-12 if dt == "float64" else 2e-5
    solve = bz.als if case["solver"] == "als" else bz.alps
    for k, (o, o2) in enumerate(zip(runs, twins)):
        for resident in (True, False):
            a = solve(*case["dev"], case["x0"], case["y0"], maxit=k + 1, subsolver=sub_factory(bz, case["gamma"]),
                      resident=resident)
            tag = (kind, shape, D, dt, "maxit=%d" % (k + 1), "resident" if resident else "host loop")
            assert (a[2], a[3], a[5]) == (o[2], o[3], o[5]) and float(a[6]) == float(o[6]), (tag, a[2:7], o[2:7])
            for e in (0, 1, 8, 9, 7):
                va, vo, v2 = (np.atleast_1d(np.asarray(v[e], np.float64)) for v in (a, o, o2))
                scale = max(float(np.max(np.abs(vo))), float(np.finfo(np.float64).tiny))          # (s of D = ZeroSet: all zero)
                dist, sens = float(np.max(np.abs(va - vo))), float(np.max(np.abs(v2 - vo)))
                print("%s %s: |device - oracle| = %.3e, sens %.3e (of the largest entry %.3e)" % (tag, NAMES[e], dist, sens, scale))
                key = (kind, dt, NAMES[e])
                w = MATRIX_WORST.get(key, (0.0, 0.0))
                MATRIX_WORST[key] = (max(w[0], dist / scale), max(w[1], sens / scale))
                assert dist <= max(base * scale, 100.0 * sens), (tag, NAMES[e], dist, sens, scale)


def test_zz_worst_distances_beside_a_matrix():
    """prints the tally of the test above (run the file whole): the worst relative distances per kind, type and quantity"""
    for key in sorted(MATRIX_WORST):
        print("%-14s %s %-13s device %.3e  oracle's twin %.3e" % (key + MATRIX_WORST[key]))
    assert MATRIX_WORST


# ------------------------------------------------------------------ (6) callback oracles: the C++ copy of the arithmetic
CALLBACK_CLASSES = [("l1", "box"), ("indbox", "zero"), ("zero", "cc")]


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("g,D", CALLBACK_CLASSES, ids=["%s-%s" % c for c in CALLBACK_CLASSES])
def test_callback_outer_loop_has_the_bits_of_the_lowered_kinds(bz, ref, monkeypatch, g, D, dt):
    """The same problems with all four oracles given as host callbacks (the oracle's own objects carry the protocol): the
    penalty and dual arithmetic then runs in the C++ copy inside alps() instead of k_penalty_init / k_dual_update.
    Expected: the bits of the lowered run."""
    _clear(monkeypatch)
    case, regime, n = table_case(g, D, dt, "adjacent", bz=bz, ref=ref)
    theta = class_theta(g, D)
    prob = bz.Problem(*case["orc"], n, n, np.dtype(dt))
    try:
        assert prob.generic
        for k in range(1, K_OUTER + 1):
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                low = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=theta)
                a = bz.alps(*case["orc"], case["x0"], case["y0"], maxit=k, subsolver=sub_factory(bz), theta_penalty=theta,
                            problem=prob)
            assert_state(a, as_state(low), (g, D, dt, regime, n, "maxit=%d" % k))
    finally:
        prob.close()


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("mode", ["finite", "nan_y", "nan_x"])
def test_callback_outer_loop_with_special_arguments(bz, ref, monkeypatch, dt, mode):
    """... and the arguments where the arithmetic branches, NaN multipliers and NaN distances included"""
    _clear(monkeypatch)
    g, D = "zero", "box"
    n = SPECIAL_N[(dt, False)]
    case = special_outer_case(g, D, dt, n, mode, bz=bz, ref=ref)
    for maxit in ((1,) if mode == "finite" else (1, 2)):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            low = bz.alps(*case["dev"], case["x0"], case["y0"], maxit=maxit, subsolver=sub_factory(bz))
            a = bz.alps(*case["orc"], case["x0"], case["y0"], maxit=maxit, subsolver=sub_factory(bz), resident=True)
        assert_state(a, as_state(low), (g, D, dt, mode, "maxit=%d" % maxit))
