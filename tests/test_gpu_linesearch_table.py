"""The step-size loop at its limit on the device: every case of tests/test_linesearch_host.py (max_backtracks 1, 2 and 3, and
20 for the two runs of the family table that exhaust it) in every form of its path, state by state
  - against the oracle over the range of states the host file proves settled: the counts (tau backtracks, gamma halvings,
    skipped pairs), tau and gamma equal exactly, x and z within the bound of the path's own table.  (Both sides start
    from one step size: the device is given the oracle's Lipschitz estimate as `gamma` with adaptive=True, which is what
    the oracle itself starts halving from.  The device's own estimate is a ratio of two reduced norms and differs from it
    by an ulp in one case in four — measured: up to 3.0e-16 in fp64, 1.3e-7 in fp32 — which the other tables hold to
    1e-13 / 1e-5; here it would only hide whether every halving is the oracle's);
  - form against form: every form gives the bits of the path's first form after every step, counts included;
  - after a step that ends at tau = 0 the new x is the previous state's z bit for bit (0 * x_d + 1 * z), in every form;
  - the tau-backtracked passes of the one-pass families take the TRIAL instantiation, plain ones TRIAL=0, and with
    BZ_TRIALFUSE=0 none does.
The host file holds the cases, the oracle's side and the proof that each case contains the events it claims."""
import warnings

import numpy as np
import pytest

from tests.test_gpu_directions_table import FLOOR32
from tests.test_gpu_families import SCALARS
from tests.test_gpu_parity import _err, iter_tol, make_cfg2
from tests.test_linesearch_host import CASE, CASES, case_ids, pair_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KNOBS = ("BZ_XR", "BZ_UNI", "BZ_GFC", "BZ_GRID", "BZ_TRIALFUSE", "BZ_FAMRT", "BZ_SPEC", "BZ_NT", "BZ_SKIPZ", "BZ_GATE", "BZ_SLACKFAST",
         "BZ_SLACKKIND", "BZ_STENCIL_REGX", "BZ_AFFINE_BLEND", "BZ_DENSE_FUSED", "BZ_GEMV_VALU", "BZ_XDNT", "BZ_SUC_GRID")
PIN = {"BZ_GFC": "2", "BZ_GRID": "512"}          # one summation tree for every form, as the tables pin it
ONE_PASS = [("xr2", dict(PIN, BZ_XR="2"), None), ("famrt", dict(PIN, BZ_XR="2", BZ_FAMRT="1"), None),
            ("spec0", dict(PIN, BZ_XR="2", BZ_SPEC="0"), None), ("xr0", dict(PIN, BZ_XR="0"), None),
            ("trialfuse0", dict(PIN, BZ_XR="2", BZ_TRIALFUSE="0"), None), ("chain", dict(PIN), False), ("nt", dict(PIN, BZ_XR="2", BZ_NT="1"), None)]
# (name, environment, fuse) per path; the first form is the base the others are held to
FORMS = {
    "headline": ONE_PASS, "family": ONE_PASS,
    "family1030": [f for f in ONE_PASS if f[0] in ("xr2", "xr0", "chain")],
    "slack": [("fast", dict(PIN, BZ_XR="2"), None), ("slackfast0", dict(PIN, BZ_XR="2", BZ_SLACKFAST="0"), None),
              ("slackkind0", dict(PIN, BZ_XR="2", BZ_SLACKKIND="0"), None), ("pairs", dict(PIN, BZ_XR="0"), None)],
    "stencil": [("regx1", {"BZ_STENCIL_REGX": "1"}, True), ("regx0", {"BZ_STENCIL_REGX": "0"}, True), ("chain", {"BZ_STENCIL_REGX": "1"}, False)],
    "dense": [("blend1-fused1", {"BZ_AFFINE_BLEND": "1", "BZ_DENSE_FUSED": "1"}, None), ("blend0-fused1", {"BZ_AFFINE_BLEND": "0", "BZ_DENSE_FUSED": "1"}, None),
              ("blend1-fused0", {"BZ_AFFINE_BLEND": "1", "BZ_DENSE_FUSED": "0"}, None), ("blend0-fused0", {"BZ_AFFINE_BLEND": "0", "BZ_DENSE_FUSED": "0"}, None)],
    "sparse_c": [("default", {}, None)], "sparse_ls": [("default", {}, None)],
    "anderson": [("default", dict(PIN), None), ("xr0", dict(PIN, BZ_XR="0"), None)],
    "broyden": [("default", dict(PIN), None), ("xr0", dict(PIN, BZ_XR="0"), None)],
}
# the base tolerance of x and z per path: iter_tol / FLOOR32 where the path's table uses the project's rule (family, ALS,
# stencil and directions tables), 1e-9 / 5e-5 for a dense or sparse matrix (tests/test_gpu_dense.py, tests/test_gpu_sparse.py,
# tests/test_gpu_sparse_least_squares.py), each widened to 100 x the oracle's own rounding sensitivity
MATRIX_PATHS = ("dense", "sparse_c", "sparse_ls")
# dense c: the four forms sum in different orders (tests/test_gpu_dense.py holds them to rounding), so each is held to the
# oracle itself.  What is bit for bit there: at max_backtracks = 2 the one backtrack is the tau = 0 one, its blended images are
# 0 * (images of x_d) + 1 * (the state's z images), so the blended and the evaluated backtrack under one BZ_DENSE_FUSED give
# the same x, z, res and scalars up to and through the first step that ends at tau = 0.  (Later states differ in the last
# bits: an image of z that was evaluated at z as a trial's forward-backward point and one evaluated at x = z come from
# different kernels.  Measured: 257 x 1028 from state 16 on, 64 x 512 never in 40 states.)
STENCIL_SCALARS = ("gamma", "f_x", "g_z", "dot_grad_res", "ss_res", "stop_norm", "last_ys", "lbfgs_H", "al_z")


def tol_of(case, sens):
    fp64 = case.dtype == np.float64
    if case.path in MATRIX_PATHS:
        return max(1e-9 if fp64 else 5e-5, 100 * sens)
    return iter_tol(sens) if fp64 else max(FLOOR32, 100 * sens)


def _begin(bz, case, built, env, fuse, monkeypatch, gamma):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev, orc, n, ny, mu, y, x0 = built
    prob = bz.Problem(*dev, n, ny, case.dtype, slack=case.slack)
    prob.set_multipliers(mu, y)
    kw = dict(case.kw, gamma=float(gamma), adaptive=True)
    if fuse is not None:
        kw["fuse"] = fuse
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(case.dtype).eps), max_backtracks=case.M,
                                  directions=case.directions(bz), **kw).c_opts(), x0)
    return prob


def _state(prob):
    st, p = prob.panoc_stats(), prob.profile2()["k_fused_iterates"]
    return (prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_scalars(),
            (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips, st.n_fused_iters, st.n_affine_blends), (p["form"], p["launches"]))


_RUNS = {}


def device_runs(bz, ref, monkeypatch, case):
    """every form of the case's path in lockstep: runs[form][j] is state j + 1 (x, z, res, scalars, counts, one-pass form and
    launches); computed once per case"""
    if case.name not in _RUNS:
        built = case.build(bz, ref)
        forms = FORMS[case.path]
        gamma = pair_of(bz, ref, case).o.gamma_start
        probs = []
        try:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for name, env, fuse in forms:
                    probs.append(_begin(bz, case, built, env, fuse, monkeypatch, gamma))
                runs = [[_state(p)] for p in probs]
                for _ in range(case.states - 1):
                    for p, r in zip(probs, runs):
                        p.panoc_step()
                        r.append(_state(p))
        finally:
            for p in probs:
                p.close()
        _RUNS[case.name] = {f[0]: r for f, r in zip(forms, runs)}
    return _RUNS[case.name]


@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_base_form_follows_the_oracle_over_the_compared_range(bz, ref, monkeypatch, case):
    """Prints the worst error / tolerance of the case; NEXT.md ("Line search at its limit") keeps the figures measured on
    an MI355X per path."""
    pair = pair_of(bz, ref, case)
    runs = device_runs(bz, ref, monkeypatch, case)
    o, t = pair.o, pair.t
    # (dense c: the four forms sum in different orders and agree to rounding only — each is held to the oracle itself)
    for name in [f[0] for f in FORMS[case.path]][:None if case.path == "dense" else 1]:
        base = runs[name]
        sens = worst = 0.0
        bt, hv, sk = 0, o.start_halvings, 0
        for j in range(pair.compared):          # state j + 1
            x, z, res, sc, cnt, _ = base[j]
            xo, zo, go = o.states[j]
            if j:
                s = o.steps[j - 1]
                bt, hv, sk = bt + s.nbt, hv + s.halvings, sk + (0 if s.kept else 1)
                assert sc["tau"] == s.tau and sc["n_backtracks"] == s.nbt, (case.name, name, j + 1, sc["tau"], s.tau, sc["n_backtracks"], s.nbt)
            assert cnt[:3] == (bt, hv, sk), (case.name, name, j + 1, cnt, (bt, hv, sk))
            assert sc["gamma"] == go, (case.name, name, j + 1, sc["gamma"], go)
            sens = max(sens, _err(t.states[j][0], xo), _err(t.states[j][1], zo))
            tol = tol_of(case, sens)
            ex, ez = _err(x, xo), _err(z, zo)
            worst = max(worst, ex / tol, ez / tol)
            assert ex <= tol and ez <= tol, f"{case.name} {name}: iterate mismatch at state {j + 1}: {ex} {ez} (tol {tol}, sens {sens})"
        print(f"{case.name} {name}: {pair.compared} states compared, worst error / tolerance {worst:.3e}, final sens {sens:.3e}, counts {(bt, hv, sk)}")
    for c in case.claims:          # the events happened on the device too: its counts and tau are the oracle's over the range
        assert pair.events[c]


TAU_CASES = [c for c in CASES if c.M >= 2]          # (max_backtracks = 1: tau stays 1)


@pytest.mark.parametrize("case", TAU_CASES, ids=case_ids(TAU_CASES))
def test_x_after_a_tau_zero_step_is_the_previous_z(bz, ref, monkeypatch, case):
    """needs no oracle: k_blend forms 0 * x_d + 1 * z.  Over the whole run, in every form."""
    seen = 0
    for name, r in device_runs(bz, ref, monkeypatch, case).items():
        for j in range(1, len(r)):
            if r[j][3]["tau"] == 0.0 and r[j][4][0] > r[j - 1][4][0]:
                assert np.array_equal(r[j][0], r[j - 1][1]), (case.name, name, j + 1)
                seen += 1
    if set(case.claims) & set("ad"):
        assert seen >= 1, case.name


def _same_bits(case, base, other, label, scalars):
    for j, (a, b) in enumerate(zip(other, base)):
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v, equal_nan=True), (case.name, label, "state", j + 1)
        for key in scalars:
            assert a[3][key] == b[3][key] or (np.isnan(a[3][key]) and np.isnan(b[3][key])), (case.name, label, "state", j + 1, key, a[3][key], b[3][key])
        assert a[4][:3] == b[4][:3], (case.name, label, "state", j + 1, a[4], b[4])


@pytest.mark.parametrize("case", [c for c in CASES if len(FORMS[c.path]) > 1], ids=case_ids([c for c in CASES if len(FORMS[c.path]) > 1]))
def test_forms_give_the_same_bits_from_the_first_step(bz, ref, monkeypatch, case):
    runs = device_runs(bz, ref, monkeypatch, case)
    names = [f[0] for f in FORMS[case.path]]
    base = runs[names[0]]
    if case.path == "dense":
        # the counts and tau of every form are the base's over the compared range; a first backtrack went onto blended images
        # where that is switched on (max_backtracks = 2: it is the tau = 0 one, whose images are the state's z images — the
        # new x is that z bit for bit, test_x_after_a_tau_zero_step_is_the_previous_z) and nowhere else
        compared = pair_of(bz, ref, case).compared
        for name in names[1:]:
            for j, (a, b) in enumerate(zip(runs[name][:compared], base)):
                assert a[4][:3] == b[4][:3] and a[3]["tau"] == b[3]["tau"], (case.name, name, j + 1, a[4], b[4])
        for name in names:
            blends = runs[name][-1][4][4]
            print(case.name, name, "blended backtracks", blends, "backtracks", runs[name][-1][4][0])
            assert (blends >= 1) if (name.startswith("blend1") and case.M >= 2 and runs[name][-1][4][0]) else blends == 0, (case.name, name, blends)
        if case.M == 2:
            # the first step that ends at tau = 0 went onto blended images (the blend count rose in it): bit for bit the
            # evaluated backtrack, every state up to and including the one after that step
            for fused in ("fused1", "fused0"):
                a, b = runs["blend1-" + fused], runs["blend0-" + fused]
                first = [j for j in range(1, len(a)) if a[j][3]["tau"] == 0.0 and a[j][4][0] > a[j - 1][4][0]]
                assert first and a[first[0]][4][4] == a[first[0] - 1][4][4] + 1, (case.name, fused, first)
                _same_bits(case, b[:first[0] + 1], a[:first[0] + 1], "blend, " + fused, SCALARS + ("tau",))
        return
    scalars = (STENCIL_SCALARS if case.path == "stencil" else SCALARS) + ("tau",)
    for name in names[1:]:
        _same_bits(case, base, runs[name], name, scalars)


ONE_PASS_CASES = [c for c in CASES if c.path in ("headline", "family")]


@pytest.mark.parametrize("case", ONE_PASS_CASES, ids=case_ids(ONE_PASS_CASES))
def test_tau_backtracked_passes_take_the_trial_instantiation(bz, ref, monkeypatch, case):
    """From the form of a step's last one-pass launch (profile2): a step whose backtrack count rose, without a halving,
    behind an iterate-history first trial shows TRIAL=1 (headline kernel) or TRIAL=-1,FAM= (a family's run-time entry) and
    one launch per trial; a step with one launch, no backtrack and no halving shows TRIAL=0; with BZ_TRIALFUSE=0 no step
    shows a trial-given form and no step launches twice.  (A step whose first trial was not an iterate-history launch —
    the ring is refilling after a skipped pair or a halving — finishes in the generic kernels by design.)"""
    runs = device_runs(bz, ref, monkeypatch, case)
    fam_headline = case.name.startswith("headline")
    marker = ",TRIAL=1" if fam_headline else ",TRIAL=-1,FAM="
    r = runs["xr2"]
    given = plain = 0
    for j in range(1, len(r)):
        dl = r[j][5][1] - r[j - 1][5][1]
        dbt, dhv = r[j][4][0] - r[j - 1][4][0], r[j][4][1] - r[j - 1][4][1]
        form = r[j][5][0]
        if dbt >= 1 and dhv == 0 and dl >= 1:
            # a step whose backtrack count rose behind an iterate-history first trial: every backtracked point went
            # through the trial-given pass, none fell to the generic kernels
            assert dl == 1 + dbt and form.startswith("k_fused_compact<XR=2") and marker in form, (case.name, j + 1, dl, dbt, form)
            given += 1
        elif dl >= 2:
            assert dbt >= 1 and form.startswith("k_fused_compact<XR=2") and marker in form, (case.name, j + 1, dl, dbt, form)
            given += 1
        elif dl == 1 and dbt == 0 and dhv == 0:
            assert ",TRIAL=0" in form, (case.name, j + 1, form)
            plain += 1
    r0 = runs["trialfuse0"]
    for j in range(1, len(r0)):
        assert r0[j][5][1] - r0[j - 1][5][1] <= 1, (case.name, j + 1)
        assert ",TRIAL=1" not in r0[j][5][0] and ",TRIAL=-1" not in r0[j][5][0], (case.name, j + 1, r0[j][5][0])
    print(f"{case.name}: {given} steps through the trial-given pass, {plain} plain one-pass steps")
    assert plain >= 1, case.name
    if set(case.claims) & set("ac") and not case.free:      # (a case that ends steps at tau = 0 sends some through that pass)
        assert given >= 1, case.name


def test_gated_blocks_equal_single_steps_through_exhausted_steps(bz, ref, monkeypatch):
    """The headline family, fp64, max_backtracks = 2, the one run with gated launches: panoc_steps in blocks against
    panoc_step, bit for bit at every block's end; no gate fallback; a pre-launched pass is released only into a step that
    accepts its first trial, so every step that ends at tau = 0 withdrew its pass."""
    case = CASE["headline-1031-f64-M2"]
    built = case.build(bz, ref)
    blocks = (1, 7, 12, 19)
    gamma = pair_of(bz, ref, case).o.gamma_start
    single = _begin(bz, case, built, {"BZ_GATE": "1"}, None, monkeypatch, gamma)
    block = _begin(bz, case, built, {"BZ_GATE": "1"}, None, monkeypatch, gamma)
    try:
        first_trial = 0
        for b in blocks:
            block.panoc_steps(b)
            for _ in range(b):
                before = single.panoc_stats()
                single.panoc_step()
                after = single.panoc_stats()
                first_trial += after.n_backtracks == before.n_backtracks and after.n_gamma_halvings == before.n_gamma_halvings
            a, c = _state(single), _state(block)
            for u, v in zip(a[:3], c[:3]):
                assert np.array_equal(u, v), b
            for key in SCALARS + ("tau", "k"):
                assert a[3][key] == c[3][key], (b, key)
            assert a[4][:3] == c[4][:3], (a[4], c[4])
        st, s1 = block.panoc_stats(), single.panoc_stats()
        print("gated", st.n_gated_launches, "aborts", st.n_gate_aborts, "fallbacks", st.n_gate_fallbacks, "backtracks", st.n_backtracks,
              "steps accepted at their first trial", first_trial)
        assert st.n_gate_fallbacks == 0 and s1.n_gated_launches == 0
        assert st.n_backtracks >= 5                                   # (max_backtracks = 2: each of them a step ending at tau = 0)
        assert 1 <= st.n_gated_launches <= first_trial                # released only into steps that accept their first trial
        # (a step that ends at tau = 0 withdraws the pass launched for it; the first step of a block has none)
        assert st.n_gate_aborts >= st.n_backtracks - len(blocks), (st.n_gate_aborts, st.n_backtracks)
    finally:
        single.close()
        block.close()


def test_max_backtracks_below_one_is_refused(bz, ref):
    n = 64
    d, dev, orc = make_cfg2(bz, ref, n)
    prob = bz.Problem(*dev, n, n, np.float64)
    prob.set_multipliers(np.full(n, 0.1), np.zeros(n))
    L = bz._lib
    try:
        for m in (0, -1):
            with pytest.raises(L.BazingaHipError, match="max_backtracks must be >= 1") as e:
                prob.panoc_begin(bz.PANOCplus(max_backtracks=m).c_opts(), np.zeros(n))
            assert e.value.code == L.BZ_ERR_ARG
    finally:
        prob.close()
