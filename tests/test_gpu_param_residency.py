"""The headline pass with its invariant parameter streams q and b cache-allocating (k_fused_compact<..., PP = 1>): only the
cache bits of two loads differ from the all-non-temporal instantiation, so every iterate and scalar must be the same bit
for bit, and the form is chosen only where q and b fit the Infinity Cache (tools/probes/mall_params.hip)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("BZ_KEEPP", "BZ_NT", "BZ_GFC", "BZ_GATE", "BZ_SKIPZ", "BZ_TRIALFUSE", "BZ_XR", "BZ_FAMRT")


def _problem(bz, n, g="l1", y=None, x0=None):
    d = bz.synth.l1_quadratic(n, start=0, dtype=np.float64)
    gg = bz.NormL1(d["lam"]) if g == "l1" else bz.NormL1Box(d["lam"], u=np.full(n, 0.75))
    prob = bz.Problem(bz.DiagQuadratic(d["q"], d["b"]), gg, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])),
                      n, n, np.float64)
    prob.set_multipliers(np.full(n, 0.1), np.zeros(n) if y is None else y)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(float).eps),
                                  directions=bz.LBFGS(5, compact=True)).c_opts(), np.zeros(n) if x0 is None else x0)
    return prob


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _compare_blocks(bz, clean_env, n, y, x0, blocks, until_backtrack):
    """PP = 1 against PP = 0 on one problem, compared bit for bit after every block of 45 steps; returns the counters"""
    probs = {}
    for keep in ("1", "0"):
        clean_env.setenv("BZ_KEEPP", keep)
        clean_env.setenv("BZ_NT", "1")
        clean_env.setenv("BZ_GFC", "1")
        probs[keep] = _problem(bz, n, y=y, x0=x0)
    try:
        for block in range(blocks):
            out = {}
            for keep, prob in probs.items():
                prob.panoc_steps(45)
                st = prob.panoc_stats()
                p = prob.profile2()["k_fused_iterates"]
                out[keep] = (prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_scalars(),
                             (st.iters, st.n_grad, st.n_prox, st.n_backtracks, st.n_gamma_halvings, st.n_fused_iters,
                              st.n_lbfgs_skips, st.n_gated_launches), p["launches"], p["form"])
            (x1, z1, s1, c1, l1, f1), (x0_, z0, s0, c0, l0, f0) = out["1"], out["0"]
            assert "PP=1" in f1 and "PP=1" not in f0, (f1, f0)
            assert np.array_equal(x1, x0_) and np.array_equal(z1, z0), block
            assert all(s1[k] == s0[k] or (np.isnan(s1[k]) and np.isnan(s0[k])) for k in s0), (block, s1, s0)
            assert c1 == c0 and l1 == l0, (block, c1, c0)
            if until_backtrack and c1[3] >= 1:
                break
        return c1
    finally:
        for prob in probs.values():
            prob.close()


@pytest.mark.timeout(900)
def test_keep_params_is_bitwise_neutral_at_the_headline_size(bz, clean_env):
    """cfg 2's problem (n = 1e7) in the library's own loop (gated pre-launch and lazy z on, the defaults), non-temporal
    streams and one grid for both runs: PP = 1 against PP = 0, everything equal bit for bit after every block of 45
    steps.  (i) From bench.py's start (x0 = 0, y = 0): the passes are launched early, gated.  (ii) From a start away
    from 0 with multipliers y (as in test_gpu_families), until a τ-backtracked point has gone through the one-pass
    kernel's TRIAL instantiation — the zero start takes no backtrack in its first blocks."""
    n = 10_000_000
    c = _compare_blocks(bz, clean_env, n, None, None, 1, False)
    assert c[7] >= 10, c                                    # (gated launches)
    rng = np.random.default_rng(3)
    c = _compare_blocks(bz, clean_env, n, rng.standard_normal(n), 0.3 * rng.standard_normal(n), 8, True)
    assert c[3] >= 1, "no τ-backtracked pass in 360 steps: the TRIAL instantiation was not compared"


@pytest.mark.parametrize("n, keepp, expect", [(10_000_000, None, True), (20_000_000, None, False),
                                              (10_000_000, "0", False)],
                         ids=["n1e7-default", "n2e7-over-budget", "n1e7-forced-off"])
def test_keep_params_form_selection(bz, clean_env, n, keepp, expect):
    """By default the headline pass keeps q and b cacheable while q + b fit the budget (256 MB: n = 1e7 yes, 2e7 no);
    BZ_KEEPP=0 turns it off.  The non-temporal form is chosen by size at both n."""
    if keepp is not None:
        clean_env.setenv("BZ_KEEPP", keepp)
    prob = _problem(bz, n)
    prob.panoc_steps(8)
    form = prob.profile2()["k_fused_iterates"]["form"]
    prob.close()
    assert form.startswith("k_fused_compact<XR=2") and ",NT=1" in form, form
    assert ("PP=1" in form) == expect, form


def test_family_instantiations_keep_today_policy(bz, clean_env):
    """The family table is unchanged: a family run at the headline size (non-temporal by size) reports a form
    without PP=1, even with BZ_KEEPP=1."""
    n = 10_000_000
    clean_env.setenv("BZ_KEEPP", "1")
    prob = _problem(bz, n, g="l1box")
    prob.panoc_steps(8)
    form = prob.profile2()["k_fused_iterates"]["form"]
    prob.close()
    assert ",FAM=" in form and ",NT=1" in form and "PP=1" not in form, form
