"""The headline pass with its packs ahead streamed through a per-wave LDS ring (k_fused_compact<..., LQ = 1>): the same
chunk map, the same body and the same reduction tree as the register pipeline, so every iterate and scalar must be the
same bit for bit; the form is chosen for the non-temporal headline pass only, and BZ_LDSQ=0 turns it off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("BZ_LDSQ", "BZ_KEEPP", "BZ_NT", "BZ_GFC", "BZ_GATE", "BZ_SKIPZ", "BZ_TRIALFUSE", "BZ_XR", "BZ_FAMRT")


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


def _compare_blocks(bz, clean_env, n, y, x0, blocks, until_backtrack, steps=45):
    """LQ = 1 against LQ = 0 on one problem (non-temporal streams), bit for bit after every block of steps"""
    probs = {}
    for lq in ("1", "0"):
        clean_env.setenv("BZ_LDSQ", lq)
        clean_env.setenv("BZ_NT", "1")
        probs[lq] = _problem(bz, n, y=y, x0=x0)
    try:
        for block in range(blocks):
            out = {}
            for lq, prob in probs.items():
                prob.panoc_steps(steps)
                st = prob.panoc_stats()
                p = prob.profile2()["k_fused_iterates"]
                out[lq] = (prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_scalars(),
                           (st.iters, st.n_grad, st.n_prox, st.n_backtracks, st.n_gamma_halvings, st.n_fused_iters,
                            st.n_lbfgs_skips, st.n_gated_launches), p["launches"], p["form"])
            (x1, z1, s1, c1, l1, f1), (x0_, z0, s0, c0, l0, f0) = out["1"], out["0"]
            assert "LQ=1" in f1 and "LQ=1" not in f0, (f1, f0)
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
def test_lds_ring_is_bitwise_neutral_at_the_headline_size(bz, clean_env):
    """cfg 2's problem (n = 1e7) in the library's own loop: (i) from bench.py's start, the gated pre-launched passes;
    (ii) from a start away from 0 with multipliers y, until a τ-backtracked point has gone through the TRIAL
    instantiation of the ring form."""
    n = 10_000_000
    c = _compare_blocks(bz, clean_env, n, None, None, 1, False)
    assert c[7] >= 10, c                                    # (gated launches)
    rng = np.random.default_rng(3)
    c = _compare_blocks(bz, clean_env, n, rng.standard_normal(n), 0.3 * rng.standard_normal(n), 8, True)
    assert c[3] >= 1, "no τ-backtracked pass in 360 steps: the TRIAL instantiation was not compared"


@pytest.mark.parametrize("n", [1_000_001, 20_011], ids=["odd-1e6", "clamped-2e4"])
def test_lds_ring_is_bitwise_neutral_on_ragged_sizes(bz, clean_env, n):
    """An odd n (a ragged last pack after the ring) and an n so small that most threads start past the last full pack
    (the ring's clamped re-requests), both with a τ-backtracked pass: the same bits as the register pipeline."""
    rng = np.random.default_rng(5)
    c = _compare_blocks(bz, clean_env, n, rng.standard_normal(n), 0.3 * rng.standard_normal(n), 8, True, steps=30)
    assert c[5] >= 1, c                                     # (one-pass iterations)


@pytest.mark.parametrize("nt, ldsq, keepp, expect", [(None, None, None, True), (None, "0", None, False),
                                                     ("0", None, None, False), (None, None, "0", True)],
                         ids=["default", "knob-off", "temporal", "pp0"])
def test_lds_ring_form_selection(bz, clean_env, nt, ldsq, keepp, expect):
    """At n = 1e7 the non-temporal headline pass takes the ring form by default (with or without cacheable q / b);
    BZ_LDSQ=0 turns it off, and the temporal form (BZ_NT=0) never takes it."""
    for k, v in (("BZ_NT", nt), ("BZ_LDSQ", ldsq), ("BZ_KEEPP", keepp)):
        if v is not None:
            clean_env.setenv(k, v)
    prob = _problem(bz, 10_000_000)
    prob.panoc_steps(8)
    form = prob.profile2()["k_fused_iterates"]["form"]
    prob.close()
    assert form.startswith("k_fused_compact<XR=2"), form
    assert ("LQ=1" in form) == expect, form
    assert ("PP=1" in form) == (keepp != "0" and nt != "0"), form


def test_family_instantiations_do_not_take_the_ring(bz, clean_env):
    """The family table is unchanged: a family run at the headline size reports a form without LQ=1, even with
    BZ_LDSQ=1."""
    clean_env.setenv("BZ_LDSQ", "1")
    prob = _problem(bz, 10_000_000, g="l1box")
    prob.panoc_steps(8)
    form = prob.profile2()["k_fused_iterates"]["form"]
    prob.close()
    assert ",FAM=" in form and ",NT=1" in form and "LQ=1" not in form, form
