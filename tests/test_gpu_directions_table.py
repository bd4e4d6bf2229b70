"""`AndersonAcceleration(n)` and `Broyden()` over every path they ride, every memory and both types, state by state against
the oracle.  The cases, the oracle's side and the proof that each case contains the events it is there for live in
tests/test_directions_host.py (no GPU); this file runs the same cases on the device.

Anderson is compared with the oracle's TWIN (`AndersonTwin`: the restatement with the coefficients formed from the Gram
products by the device's own elimination), so the 1e-6 of tests/test_gpu_directions.py — normal equations against a QR
least squares — is gone: x and z are held to the project's rule, `iter_tol(sens)` in fp64 (1e-10, or 100 x the oracle's own
rounding sensitivity under `LongDoubleReducer`) and max(2e-5, 100 sens) in fp32, gamma to 1e-12 (fp32: 1e-5 while the
tolerance is still its floor).  Broyden's oracle needs no twin.  After every run the event counts of the device
(`panoc_stats`: gamma halvings, tau backtracks, skipped pairs) are the oracle's.

What compares the Broyden operator itself: the library has no read-out of the n x n matrix, so every run is continued by
one more step than its case asks for — that step's x is x - H res, the operator applied to a residual it has not seen."""
import warnings

import numpy as np
import pytest

from tests.test_directions_host import ANDERSON_CASES, BROYDEN_CASES, CASES, OracleRun, case_ids
from tests.test_gpu_families import SCALARS
from tests.test_gpu_parity import LongDoubleReducer, _err, iter_tol, make_cfg2

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

KNOBS = ("BZ_XR", "BZ_UNI", "BZ_GFC", "BZ_GRID", "BZ_TRIALFUSE", "BZ_FAMRT", "BZ_NT", "BZ_SKIPZ", "BZ_GEMV_VALU",
         "BZ_STENCIL_REGX")
FLOOR32 = 2e-5          # the floor of the fp32 cases of tests/test_gpu_family_table.py


def _clear(monkeypatch, env=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _begin(bz, case, built, fuse=None):
    dev, orc, n, ny, mu, y, x0 = built
    prob = bz.Problem(*dev, n, ny, case.dtype, slack=case.slack)
    prob.set_multipliers(mu, y)
    sub = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(case.dtype).eps),
                       fuse=case.fuse if fuse is None else fuse, directions=case.directions(bz), **case.kw)
    prob.panoc_begin(sub.c_opts(), x0)
    return prob


def trace(bz, ref, case, extra=0):
    """the device, the oracle (twin / probe) and the oracle under LongDoubleReducer side by side for case.iters + extra
    states: rows (k, err_x, err_z, gamma_dev, gamma_ref, fused, sens), the one-pass form after every step, the device's
    stats and the oracle's run"""
    built = case.build(bz, ref)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prob = _begin(bz, case, built)
        try:
            runs = [OracleRun(ref, case, built), OracleRun(ref, case, built, reducer=LongDoubleReducer())]
            rows, forms, sens = [], [], 0.0
            iters = case.iters + extra
            for k in range(iters):
                st = runs[0].st
                sc = prob.panoc_scalars()
                sens = max(sens, _err(runs[1].st.x, st.x), _err(runs[1].st.z, st.z))
                rows.append((k + 1, _err(prob.panoc_vector("x"), st.x), _err(prob.panoc_vector("z"), st.z), sc["gamma"],
                             float(st.gamma), sc["fused"], sens))
                if k + 1 < iters:
                    prob.panoc_step()
                    forms.append(prob.profile2()["k_fused_iterates"]["form"])
                    runs[0].step()
                    runs[1].step()
            stats = prob.panoc_stats()
        finally:
            prob.close()
    return rows, forms, stats, runs[0]


def check(case, rows, stats, run, label=""):
    """the tolerances of the module docstring on every state, then the event counts; prints the worst error / tolerance"""
    fp64 = case.dtype == np.float64
    worst, floor_states, tight = 0.0, 0, 0
    for k, ex, ez, g_d, g_r, fused, sens in rows:
        if fp64:
            tol = iter_tol(sens)
            assert abs(g_d - g_r) <= 1e-12 * g_r, (case.name, label, k, g_d, g_r)
            floor_states += tol == 1e-10
        else:
            tol = max(FLOOR32, 100 * sens)
            if tol == FLOOR32:
                assert abs(g_d - g_r) <= 1e-5 * g_r, (case.name, label, k, g_d, g_r)
            floor_states += tol == FLOOR32
        tight += tol <= (1e-10 if fp64 else 1e-3)
        worst = max(worst, ex / tol, ez / tol)
        assert ex <= tol and ez <= tol, f"{case.name} {label}: iterate mismatch at k={k}: {ex} {ez} (tol {tol}, sens {sens})"
    counts = run.counts()
    print(f"{case.name} {label}: worst error / tolerance {worst:.3e}; {floor_states} of {len(rows)} states at the floor; "
          f"final sens {rows[-1][6]:.3e}; halvings {stats.n_gamma_halvings} backtracks {stats.n_backtracks} "
          f"skips {stats.n_lbfgs_skips} one-pass {stats.n_fused_iters}; oracle {counts}")
    # the widened tolerance may not carry the comparison (the rule of tests/test_gpu_family_table.py): fp64, two states in
    # three are held to the floor itself; fp32, where the oracle's two roundings part by 1e-7..1e-6 within a few states, one
    # in three to 1e-3
    assert tight >= (len(rows) * 2 // 3 if fp64 else len(rows) // 3), (case.name, label, tight)
    # the device's counts are the oracle's, in both types; and the events the case is there for happened on the device
    assert stats.n_gamma_halvings == run.st.n_gamma_halvings, (case.name, label, stats.n_gamma_halvings, counts)
    assert stats.n_backtracks == counts["backtrack"], (case.name, label, stats.n_backtracks, counts)
    if "halving" in case.claims:
        assert stats.n_gamma_halvings - counts["start_halvings"] >= 1, (case.name, label, stats.n_gamma_halvings, counts)
    if "backtrack" in case.claims:
        assert stats.n_backtracks >= 1, (case.name, label, stats.n_backtracks)
    if case.kind == "anderson":
        assert stats.n_lbfgs_skips == 0, (case.name, label, stats.n_lbfgs_skips)      # every pair is kept
        assert stats.n_affine_images == 0                                               # no affine images with this direction


# ------------------------------------------------------------------------------------------------------ Anderson
@pytest.mark.parametrize("case", ANDERSON_CASES, ids=case_ids(ANDERSON_CASES))
def test_anderson_follows_the_twin(bz, ref, monkeypatch, case):
    """Every Anderson case, 14 to 18 states.  Measured on an MI355X, worst (error / tolerance) over the states of a case,
    and how many states were held to the floor itself (1e-10 / 2e-5):
      headline m1 / m2 / m3 / m5, fp64     6.5e-6 / 1.9e-5 / 7.8e-6 / 2.5e-5   14 of 14 each
      headline m1 / m2 / m3 / m5, fp32     1.1e-2 / 1.1e-2 / 1.2e-2 / 1.4e-2    2 of 14 each (oracle's roundings 4e-7 .. 4e-6 apart;
                                           the halving and backtrack counts are the oracle's all the same)
      indboxvec-boxvec m5 fp64 / m2 fp32   4.1e-5 (14 of 14) / 2.3e-2 (8 of 14)
      l1-vc n62 / zero-vc n502 / l1-xor m5 3.5e-4 / 1.2e-5 / 1.4e-5, every state;  l1-xor m3 fp32 8.6e-3 (5 of 16)
      chain m2 fp64 / m5 fp32              1.9e-5 (14 of 14) / 1.4e-2 (2 of 14)
      stencil 33x46                        5.4e-6 (14 of 14)
      dense 20x100 m5 fp64 / m2 fp32       4.2e-4 (14 of 14) / 1.1e-1 (8 of 14)
      dense 64x512 m3 fp64 / m5 fp32       4.0e-5 (14 of 14) / 8.1e-3 (9 of 14)
      sparse 300x100                       4.2e-5 (14 of 14)
      l21 / lpnonneg / slack / halving     1.0e-5 / 1.8e-5 / 9.5e-6 / 1.4e-5, every state
    i.e. in fp64 the device is 1e-15 .. 4e-14 from the twin where the 1e-6 of tests/test_gpu_directions.py used to stand."""
    _clear(monkeypatch)
    rows, forms, stats, run = trace(bz, ref, case)
    check(case, rows, stats, run)
    one_pass = case.fuse and not case.slack and case.name.split("-")[0] in ("headline", "indboxvec", "l1", "zero", "halving")
    if one_pass:
        # the one-pass kernels served the iterations, and in the iterate-history form once the memory was full
        assert sum(r[5] for r in rows) >= len(rows) // 2, [r[5] for r in rows]
        assert any(f.startswith("k_fused_compact<XR=2") for f in forms[case.param:]), sorted(set(forms))
    if "nonpos" in case.claims:
        assert run.counts()["nonpos"] >= 1
    if not case.fuse:
        assert sum(r[5] for r in rows) == 0


def _lockstep(bz, ref, monkeypatch, case, configs):
    """the same case under several (environment, fuse) configurations, state by state: x, z, res, the scalars, the
    counters and the one-pass form after every step"""
    built = case.build(bz, ref)
    probs, runs = [], [[] for _ in configs]
    try:
        for env, fuse in configs:
            _clear(monkeypatch, env)
            probs.append(_begin(bz, case, built, fuse=fuse))
        for _ in range(case.iters - 1):
            for prob, r in zip(probs, runs):
                prob.panoc_step()
                st = prob.panoc_stats()
                r.append((prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_scalars(),
                          (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips, st.n_fused_iters),
                          prob.profile2()["k_fused_iterates"]["form"]))
    finally:
        for prob in probs:
            prob.close()
    return runs


def _same_bits(case, base, other, label, scalars=SCALARS):
    for k, (a, b) in enumerate(zip(other, base)):
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v, equal_nan=True), (case.name, label, k + 1)
        for key in scalars:
            assert a[3][key] == b[3][key] or (np.isnan(a[3][key]) and np.isnan(b[3][key])), (case.name, label, k + 1, key)
        assert a[4][:3] == b[4][:3], (case.name, label, k + 1, a[4], b[4])


PIN = {"BZ_GFC": "2", "BZ_GRID": "512"}


@pytest.mark.parametrize("name", ["headline-m3-f64", "headline-m2-f32", "headline-m5-f32", "l1-vc-n62-m3-f64",
                                  "zero-vc-n502-m3-f64", "l1-xor-m3-f32"])
def test_anderson_forms_are_bitwise_neutral(bz, ref, monkeypatch, name):
    """The stored-pair form (BZ_XR=0), the iterate-history form and (headline) the run-time instantiation (BZ_FAMRT=1) on
    one pinned grid give the same bits under Anderson — through tau backtracks (the TRIAL instantiation), a gamma halving,
    and, with a pairwise D, through kept pairs with <s, y> <= 0: the iterate-history form goes on through them."""
    case = CASES[name]
    configs = [(dict(PIN, BZ_XR="0", BZ_TRIALFUSE="0"), None), (dict(PIN, BZ_XR="2", BZ_TRIALFUSE="1"), None)]
    if name.startswith("headline"):
        configs.append((dict(PIN, BZ_XR="2", BZ_FAMRT="1", BZ_TRIALFUSE="1"), None))
    with np.errstate(all="ignore"):
        base, *others = _lockstep(bz, ref, monkeypatch, case, configs)
    assert not any(b[5].startswith("k_fused_compact<XR=2") for b in base), base[-1][5]
    for (env, _), r in zip(configs[1:], others):
        _same_bits(case, base, r, env)
        forms = [a[5] for a in r]
        assert any(f.startswith("k_fused_compact<XR=2") for f in forms[case.param:]), sorted(set(forms))
        assert r[-1][4][2] == 0                      # no pair skipped
        if "nonpos" in case.claims:
            # the iterate-history form is still what runs after the pair with <s, y> <= 0 (last_ys of that state)
            at = [k for k, a in enumerate(r) if not a[3]["last_ys"] > 0]
            assert at, "no pair with <s, y> <= 0 on the device"
            # (a following step that halves gamma or backtracks tau is not one pass whatever the pair was)
            plain = [k for k in at if k + 1 < len(r) and r[k + 1][4][:2] == r[k][4][:2]]
            assert plain or name != "l1-vc-n62-m3-f64", (at, [a[4] for a in r])
            for k in plain:
                assert forms[k + 1].startswith("k_fused_compact<XR=2"), (k, forms)
                assert r[k + 1][4][3] == r[k][4][3] + 1          # (... as a one-pass iteration)
        if "backtrack" in case.claims and "BZ_FAMRT" not in env:
            # The tau-backtracked passes took the TRIAL instantiation.  Only this configuration can tell: under BZ_FAMRT=1
            # every pass, plain or trial, is the run-time instantiation and is labelled TRIAL=-1.  Here a plain pass is
            # TRIAL=0 (the headline kernel and the family's compile-time entry alike) and a trial-given pass TRIAL=1
            # (headline kernel) or TRIAL=-1 (the family's run-time entry).  The form is that of a step's LAST one-pass
            # launch, which in a step whose backtrack count rose is its last trial-given pass.
            trial = ",TRIAL=1" if name.startswith("headline") else ",TRIAL=-1,FAM="
            bt = [0] + [a[4][0] for a in r]
            hv = [r[0][4][1]] + [a[4][1] for a in r]
            rose = [k for k in range(len(r)) if bt[k + 1] > bt[k]]
            print(name, env, [(k, a[4][:2], forms[k]) for k, a in enumerate(r)])
            assert rose, bt
            for k in rose:
                assert forms[k].startswith("k_fused_compact<XR=2") and trial in forms[k], (k, forms[k], bt)
            for k in range(case.param + 1, len(r)):
                fused_rose = r[k][4][3] > r[k - 1][4][3]      # (a step without a one-pass launch repeats the previous form)
                if k not in rose and hv[k + 1] == hv[k] and fused_rose and forms[k].startswith("k_fused_compact<XR=2"):
                    assert ",TRIAL=0" in forms[k], (k, forms[k])


@pytest.mark.parametrize("name", ["stencil-33x46-m3"])
def test_anderson_stencil_fast_path_equals_the_generic_kernels_bitwise(bz, ref, monkeypatch, name):
    """the arithmetic test_stencil_fast_path_equals_generic_bitwise holds equal for the compact L-BFGS form, with Anderson's
    coefficients: fast path on, off (fuse=False), and on with res read from memory (BZ_STENCIL_REGX=0)"""
    case = CASES[name]
    configs = [({"BZ_STENCIL_REGX": "1"}, True), ({"BZ_STENCIL_REGX": "1"}, False), ({"BZ_STENCIL_REGX": "0"}, True)]
    base, *others = _lockstep(bz, ref, monkeypatch, case, configs)
    keys = ("gamma", "f_x", "g_z", "dot_grad_res", "ss_res", "stop_norm", "last_ys", "lbfgs_H", "al_z")
    for (env, fuse), r in zip(configs[1:], others):
        _same_bits(case, base, r, (env, fuse), scalars=keys)
    assert all(a[3]["lbfgs_H"] == 1.0 for a in base)          # H is pinned to 1 under Anderson


def test_anderson_keeps_H_at_one_and_takes_no_affine_images(bz, ref, monkeypatch):
    """dense c with D = ZeroSet is where L-BFGS tracks affine images: Anderson takes none, and its H stays 1 in every
    state, through the redo path of a halving too"""
    _clear(monkeypatch)
    for name in ("dense-20x100-m5-f64", "halving-m3-f64"):
        case = CASES[name]
        prob = _begin(bz, case, case.build(bz, ref))
        try:
            for _ in range(case.iters - 1):
                prob.panoc_step()
                assert prob.panoc_scalars()["lbfgs_H"] == 1.0
            st = prob.panoc_stats()
            assert st.n_affine_images == 0 and st.n_affine_blends == 0 and st.n_lbfgs_skips == 0
        finally:
            prob.close()


def test_direction_refusals(bz, ref):
    for m in (0, 6):
        with pytest.raises(bz.UnsupportedOracle, match="1 <= n <= 5"):
            bz.AndersonAcceleration(m)
    n = 64
    d, dev, orc = make_cfg2(bz, ref, n)
    prob = bz.Problem(*dev, n, n, np.float64)
    prob.set_multipliers(np.full(n, 0.1), np.zeros(n))
    L = bz._lib
    try:
        for mem, dirs, code, msg in ((0, L.BZ_DIR_ANDERSON, L.BZ_ERR_ARG, "1 <= n <= 5"), (6, L.BZ_DIR_ANDERSON, L.BZ_ERR_ARG, "1 <= n <= 5"),
                                     (5, 7, L.BZ_ERR_ARG, "unknown `directions`")):
            o = bz.PANOCplus(directions=bz.AndersonAcceleration(3)).c_opts()
            o.lbfgs_memory, o.directions = mem, dirs
            with pytest.raises(L.BazingaHipError, match=msg) as e:
                prob.panoc_begin(o, np.zeros(n))
            assert e.value.code == code
    finally:
        prob.close()
    n = 4097
    d, dev, orc = make_cfg2(bz, ref, n)
    prob = bz.Problem(*dev, n, n, np.float64)
    prob.set_multipliers(np.full(n, 0.1), np.zeros(n))
    try:
        with pytest.raises(L.BazingaHipError, match="n <= 4096") as e:
            prob.panoc_begin(bz.PANOCplus(directions=bz.Broyden()).c_opts(), np.zeros(n))
        assert e.value.code == L.BZ_ERR_UNSUPPORTED
    finally:
        prob.close()


@pytest.mark.parametrize("dt,n", [("float64", 4001), ("float32", 4003)])
def test_anderson_whole_alps_ends_where_lbfgs_ends(bz, ref, dt, n):
    dtype = np.dtype(dt).type
    d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
    x0, y0 = np.zeros(n, dtype), np.zeros(n, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = bz.alps(*dev, x0, y0, subsolver=lambda **kw: bz.PANOCplus(directions=bz.AndersonAcceleration(5), **kw))
        o = bz.alps(*dev, x0, y0)
    print(dt, a[5], o[5], a[2], o[2], a[3], o[3], float(np.max(np.abs(a[0] - o[0]))))
    assert a[5] == o[5] == "first_order" and np.max(np.abs(a[0] - o[0])) <= 2e-5


# ------------------------------------------------------------------------------------------------------- Broyden
@pytest.mark.parametrize("case", BROYDEN_CASES, ids=case_ids(BROYDEN_CASES))
def test_broyden_follows_the_oracle(bz, ref, monkeypatch, case):
    """Every Broyden case and one state more (the operator applied to one more residual).  Sizes by the plan they reach
    (tests/test_directions_host.py: test_broyden_sizes_reach_the_chunk_plans_they_are_chosen_for).  Measured on an
    MI355X, worst (error / tolerance): fp64 n = 2 exact, 63: 3.4e-5, 1030: 3.9e-6, 1031: 5.7e-5, 4096: 7.9e-6, halving 1.9e-4,
    backtrack 1.3e-2 (13 of 17 states at the floor), dense c 3.8e-5, xor 8.5e-4, the s = 0 case exact; fp32 n = 63: 3.8e-3,
    1024: 2.0e-2, 1030: 1.8e-2, 4096: 1.7e-2."""
    _clear(monkeypatch)
    rows, forms, stats, run = trace(bz, ref, case, extra=1)
    check(case, rows, stats, run)
    if "ss0" in case.claims:
        assert run.counts()["ss0"] >= 1


def test_broyden_mfma_and_valu_routes_agree(bz, ref, monkeypatch):
    """n = 1024 in fp32: s'H on the matrix cores by default, on the vector ALUs with BZ_GEMV_VALU set; both follow the
    oracle, and the two end within the tolerance of each other"""
    case = CASES["n1024-f32"]
    built = case.build(bz, ref)
    ends = []
    for env, mfma in (({}, True), ({"BZ_GEMV_VALU": "1"}, False)):
        _clear(monkeypatch, env)
        rows, forms, stats, run = trace(bz, ref, case, extra=1)
        check(case, rows, stats, run, label=str(env))
        prob = _begin(bz, case, built)
        try:
            for _ in range(case.iters - 1):
                prob.panoc_step()
            launches = prob.profile2()["k_gemv_t_mfma"]["launches"]
            assert (launches >= case.iters - 1) if mfma else launches == 0, (env, launches)
            ends.append(prob.panoc_vector("x"))
        finally:
            prob.close()
    tol = max(FLOOR32, 100 * rows[-1][6])
    assert _err(ends[1], ends[0]) <= tol


@pytest.mark.parametrize("name", ["halving-n63", "backtrack-n63"])
def test_broyden_kernel_chain_equals_the_fused_path(bz, ref, monkeypatch, name):
    """fuse=False against fuse=True through a gamma halving / tau backtracks: the operator's kernels are the same in
    both, the element-wise arithmetic is the same (test_fused_equals_generic_bitwise), so are the bits"""
    case = CASES[name]
    base, other = _lockstep(bz, ref, monkeypatch, case, [({}, True), ({}, False)])
    _same_bits(case, base, other, "fuse=False", scalars=("gamma", "f_x", "g_z", "stop_norm", "last_ys"))
    assert base[-1][4][1 if name.startswith("halving") else 0] >= 1
