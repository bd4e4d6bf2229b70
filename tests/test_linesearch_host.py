"""The step-size loop of PANOCplus at its limit, the part that needs no GPU: the table of cases that
tests/test_gpu_linesearch_table.py runs on the device, the oracle's side of each run, and the proof that the oracle alone
produces the events each case claims inside the range of states that is compared.

`max_backtracks` (M below) bounds the trials of one step.  A trial either halves gamma (f(z) above its model: the trial
is repeated with gamma / 2 and counts), or is accepted (the envelope test holds, or it is trial M), or is rejected: tau is
halved, and before trial M it is set to 0 — the trial point is then the forward-backward point z of the state the step
started from, and trial M is accepted whatever its envelope value is.  M = 1 switches the line search off.

Events of a step (`events_of`):
  (a) accepted at tau = 0: tau == 0, n_backtracks == M - 1, the last trial not a halving;
  (b) accepted before the limit: fewer than M trials;
  (c) two steps in a row that end at tau = 0;
  (d) a gamma halving inside a step that ends at tau = 0.  (A halving uses up a trial without a backtrack, so such a step
      has n_backtracks < M - 1: "exhausted" is tau == 0 here, not the count);
  (e) a gamma halving in trial M: the loop ends with gamma halved and the trial not repeated, so the residual of the new
      state belongs to the gamma before the halving;
  (f) M = 1 and the one trial fails the envelope test and is accepted;
  (g) a pair with <s, y> <= 0 (skipped by L-BFGS) at a step that ends at tau = 0.  Not asserted: see SKIPPED_AT_TAU0.

Ties.  Every decision of a step has a margin: f(z) - (f_z_upp + tol) for the halving, FBE_new - threshold for the
envelope test (which decides nothing in trial M, and is not counted there).  The oracle runs twice, with its own sums
and with `LongDoubleReducer`.  A decision is settled when both runs take the same branch and the margin exceeds 100 times
the difference of the two margins, floored at 10 eps (1 + |FBE|).  A case is compared up to the state before its first
unsettled decision (`Pair.compared`), and must keep its anchor — the first step that ends at tau = 0; with M = 1 the first
step with event (e) or (f) — and eight states behind it inside that range.  Cases marked `free` are not held to that: the
oracle's two roundings part too early there (every candidate start tried: see FREE), or, for the two runs of the family
table that exhaust twenty backtracks, the limit is met after forty steps.  They are compared with the oracle over
whatever range is settled and are in the table for the forms, which need no oracle."""
import warnings
import zlib

import numpy as np
import pytest

from oracle import bazinga_ref as REF
from tests.test_directions_host import AndersonTwin, headline, pairs

BEHIND = 8


# ------------------------------------------------------------------------------------------------ the oracle, recording
class RecordingIteration(REF.PANOCplusIteration):
    """`PANOCplusIteration.step` restated line by line with the margins of every trial kept in `self.trials`: rows
    (k, halving margin or None, envelope margin or None, FBE_x, branch) with branch "halve", "accept" or "reject".
    test_recording_iteration_is_the_oracle holds it to the oracle's own step bit for bit."""

    def step(self, st):
        T = self.T
        self.trials = []
        st.x_prev[...] = st.x
        st.res_prev[...] = st.res
        FBE_x = self._f_model(st) + st.g_z
        st.H.mul(st.d, -st.res)
        st.tau = T(1)
        np.add(st.x, st.d, out=st.x_d)
        st.f_x_d = self.f.gradient(st.grad_f_x_d, st.x_d)
        st.x[...] = st.x_d
        st.grad_f_x[...] = st.grad_f_x_d
        st.f_x = st.f_x_d
        st.z_curr[...] = st.z
        sigma = self.beta * (T(0.5) / st.gamma) * (T(1) - self.alpha)
        tol = T(10) * self.eps * (T(1) + abs(FBE_x))
        nr = REF._norm(st.res)
        threshold = FBE_x - sigma * (nr * nr) + tol
        st.n_backtracks = 0
        for k in range(1, self.max_backtracks + 1):
            st.y[...] = st.x - st.gamma * st.grad_f_x
            st.g_z = self.g.prox(st.z, st.y, st.gamma)
            st.res[...] = st.x - st.z
            f_z_upp = self._f_model(st)
            mh = None
            if self.gamma is None or self.adaptive:
                f_z = self.f.gradient(st.grad_f_z, st.z)
                st.f_z = f_z
                tol = T(10) * self.eps * (T(1) + abs(f_z))
                mh = float(f_z) - float(f_z_upp + tol)
                if f_z > f_z_upp + tol and st.gamma >= self.minimum_gamma:
                    st.gamma = st.gamma * T(0.5)
                    st.n_gamma_halvings += 1
                    sigma = sigma * T(2)
                    st.H.reset()
                    self.trials.append((k, mh, None, float(FBE_x), "halve"))
                    continue
            else:
                st.f_z = self.f.gradient(st.grad_f_z, st.z)
            FBE_x_new = f_z_upp + st.g_z
            me = float(FBE_x_new) - float(threshold)
            if FBE_x_new <= threshold or k >= self.max_backtracks:
                self.trials.append((k, mh, me, float(FBE_x), "accept"))
                break
            self.trials.append((k, mh, me, float(FBE_x), "reject"))
            st.tau = T(0) if k >= self.max_backtracks - 1 else st.tau / T(2)
            st.n_backtracks += 1
            st.x[...] = st.tau * st.x_d + (T(1) - st.tau) * st.z_curr
            st.f_x = self.f.gradient(st.grad_f_x, st.x)
        st.last_ys = st.H.update(st.x - st.x_prev, st.res - st.res_prev)
        return st


class Step:
    """what one step did: tau, n_backtracks, the halvings of the step, whether the pair was kept, the trials"""

    def __init__(self, st, halvings, trials, keeps_every_pair):
        self.tau, self.nbt, self.halvings = float(st.tau), int(st.n_backtracks), halvings
        self.ys_pos = bool(st.last_ys > 0)
        self.kept = keeps_every_pair or self.ys_pos
        self.trials = trials


class Case:
    """One run of the table.  path: the row of the device table it belongs to; build(bz, ref) -> (dev oracles, ref
    oracles, n, ny, mu, y, x0); M: max_backtracks; direction: "lbfgs", "anderson" (memory 3) or "broyden"; states: how
    many states are run (the first is the initial one); kw: the step-size keywords of both solvers; claims: the events
    (letters) that must lie inside the compared range; free: not held to the anchor rule (module docstring)."""

    def __init__(self, name, path, dt, M, build, claims="", direction="lbfgs", kw=None, slack=False, free=False, states=40):
        self.name, self.path, self.dtype, self.M, self.states = name, path, np.dtype(dt).type, M, states
        self.build, self.claims, self.direction, self.kw, self.slack, self.free = build, claims, direction, dict(kw or {}), slack, free

    def __repr__(self):
        return self.name

    def directions(self, m):
        return {"lbfgs": lambda: m.LBFGS(5), "anderson": lambda: m.AndersonAcceleration(3),
                "broyden": lambda: m.Broyden(theta_bar=0.2)}[self.direction]()


class OracleRun:
    """the oracle's iteration of a case under a reducer of the caller's: `states` (x, z, gamma of every state, copies) and
    `steps` (a Step per step; steps[j - 1] leads from state j to state j + 1, states counted from 1)"""

    def __init__(self, ref, case, built, reducer=None):
        dev, orc, n, ny, mu, y, x0 = built
        self.ref, self.reducer, self.case = ref, reducer, case
        self.states, self.steps = [], []
        ref.set_reducer(reducer)
        try:
            if case.slack:
                F = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), x0[:n])
                G = ref.NonsmoothCostFunSlack(orc[1], orc[3], n, ny)
            else:
                F, G = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0), ref.NonsmoothCostFun(orc[1])
            self.it = RecordingIteration(F, G, x0, minimum_gamma=float(np.finfo(case.dtype).eps), max_backtracks=case.M,
                                         directions=case.directions(ref), **case.kw)
            self.st = self.it.init()
            if case.direction == "anderson":      # (the device's normal equations: tests/test_directions_host.py)
                self.st.H = AndersonTwin(3, self.st.x)
            self.start_halvings = self.st.n_gamma_halvings
            # the step size the start's halvings began from (the Lipschitz estimate): exact, the halvings are by two
            self.gamma_start = self.st.gamma * case.dtype(2) ** self.start_halvings
        finally:
            ref.set_reducer(None)
        self._keep()

    def _keep(self):
        self.states.append((self.st.x.copy(), self.st.z.copy(), float(self.st.gamma)))

    def step(self):
        self.ref.set_reducer(self.reducer)
        try:
            h0 = self.st.n_gamma_halvings
            self.st = self.it.step(self.st)
        finally:
            self.ref.set_reducer(None)
        self.steps.append(Step(self.st, self.st.n_gamma_halvings - h0, self.it.trials, self.case.direction != "lbfgs"))
        self._keep()
        return self.st


def events_of(steps, M):
    """{letter: [step numbers]} over a list of Steps (step j leads from state j to state j + 1)"""
    ev = {c: [] for c in "abcdefg"}
    for j, s in enumerate(steps, 1):
        last_halved = s.trials[-1][4] == "halve"
        zero = s.tau == 0.0 and M >= 2
        if zero and s.nbt == M - 1 and not last_halved:
            ev["a"].append(j)
        if len(s.trials) < M:
            ev["b"].append(j)
        if zero and j >= 2 and steps[j - 2].tau == 0.0:
            ev["c"].append(j)
        if zero and s.halvings:
            ev["d"].append(j)
        if last_halved and s.trials[-1][0] == M:
            ev["e"].append(j)
        if M == 1 and not last_halved and s.trials[-1][2] > 0:
            ev["f"].append(j)
        if zero and not s.ys_pos:
            ev["g"].append(j)
    return ev


def settled(a, b, eps, M):
    """whether every decision of a step is settled between the oracle's Step `a` and its twin's `b` (module docstring).
    Whether the pair is kept (<s, y> > 0) has no margin of the two kinds: the two runs must agree on it."""
    if len(a.trials) != len(b.trials) or a.ys_pos != b.ys_pos:
        return False
    for (k, mh, me, fbe, br), (k2, mh2, me2, fbe2, br2) in zip(a.trials, b.trials):
        if br != br2:
            return False
        floor = 10 * eps * (1 + abs(fbe))
        margins = [(mh, mh2)] if mh is not None else []
        if br != "halve" and k < M:      # (in trial M the envelope test decides nothing)
            margins.append((me, me2))
        for m, m2 in margins:
            if not abs(m) > max(100 * abs(m - m2), floor):
                return False
    return True


class Pair:
    """the oracle and its extended-precision twin over a case's states; `compared`: the number of leading states that are
    compared with the device (the states up to the one before the first unsettled decision)"""

    def __init__(self, bz, ref, case):
        built = case.build(bz, ref)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            from tests.test_gpu_parity import LongDoubleReducer
            self.o, self.t = OracleRun(ref, case, built), OracleRun(ref, case, built, reducer=LongDoubleReducer())
            for _ in range(case.states - 1):
                self.o.step()
                self.t.step()
        eps = float(np.finfo(case.dtype).eps)
        self.case, self.compared = case, case.states
        for j, (a, b) in enumerate(zip(self.o.steps, self.t.steps), 1):
            if not settled(a, b, eps, case.M):
                self.compared = j
                break
        # (steps 1 .. compared - 1 lead to compared states)
        self.events = events_of(self.o.steps[:self.compared - 1], case.M)
        self.all_events = events_of(self.o.steps, case.M)

    def anchor(self):
        """the first step that ends at tau = 0 (M = 1: the first step with event (e) or (f)), over the whole run"""
        ev = self.all_events
        first = [s for s in ([j for j, s in enumerate(self.o.steps, 1) if s.tau == 0.0] if self.case.M >= 2 else ev["e"] + ev["f"])]
        return min(first) if first else None


_PAIRS = {}


def pair_of(bz, ref, case):
    if case.name not in _PAIRS:
        _PAIRS[case.name] = Pair(bz, ref, case)
    return _PAIRS[case.name]


# --------------------------------------------------------------------------------------------------------- the builders
# (thin: the problems are those of the existing tables' generators; what is chosen here is a size, a start and multipliers)
def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def family(n, dt, fam, regime="uni0", far=False):
    """tests/test_gpu_family_table.make_case"""
    def build(bz, ref):
        from tests.test_gpu_family_table import make_case
        dev, orc, mu, y, x0 = make_case(bz, ref, n, fam, np.dtype(dt).type, regime, far=far)
        return dev, orc, n, n, mu, y, x0
    return build


def slack(n, dt, g, D, regime="uni0", far=True, seed=""):
    """tests/test_gpu_als_table.make_slack_case: the lifted vector [x; s]"""
    def build(bz, ref):
        from tests.test_gpu_als_table import make_slack_case
        dev, orc, mu, y, xs0, _ = make_slack_case(bz, ref, n, g, D, np.dtype(dt).type, regime, far=far, seed=seed)
        return dev, orc, n, n, mu, y, xs0
    return build


def stencil(nx, ny, cls, regime="uni0", far=True):
    """tests/test_gpu_stencil_table.make_case"""
    def build(bz, ref):
        from tests.test_gpu_stencil_table import make_case
        dev, orc, mu, y, x0 = make_case(bz, ref, nx, ny, cls, np.float64, regime, far=far)
        return dev, orc, nx * ny, nx * ny, mu, y, x0
    return build


def dense_c(ny, n, dt, ys=0.1, xs=0.0, seed=0):
    """tests/test_gpu_parity.make_cfg4 (f = Zero, g = NormL1, c = Ax - b dense, D = ZeroSet), mu = 0.1"""
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg4
        dtype = np.dtype(dt).type
        d, dev, orc = make_cfg4(bz, ref, ny, n, dtype)
        rng = _rng("ls-dense", ny, n, seed)
        return dev, orc, n, ny, np.full(ny, 0.1, dtype), (ys * rng.standard_normal(ny)).astype(dtype), \
            (xs * rng.standard_normal(n)).astype(dtype)
    return build


def _structured_csr(ny, n, p, seed):
    from tests.test_gpu_sparse import csr_of, structured
    A = structured(ny, n, p, np.random.default_rng(ny * 7 + n + seed), False, np.float64)
    return A, csr_of(A, np.random.default_rng(1))


def sparse_c(ny, n, p=0.1, ys=1.0, xs=1.0, seed=0):
    """c(x) = Ax - b with A = structured / csr_of of tests/test_gpu_sparse.py beside DiagQuadratic, NormL1 and a box D"""
    def build(bz, ref):
        from tests.test_gpu_sparse import CsrOracle
        A, (indptr, indices, data) = _structured_csr(ny, n, p, seed)
        rng = _rng("ls-sparse-c", ny, n, seed)
        b = rng.standard_normal(ny)
        d = bz.synth.l1_quadratic(n)
        csr = (indptr, indices, data, b, n)
        dev = (bz.DiagQuadratic(d["q"], d["b"]), bz.NormL1(0.8), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(-1.0, 1.0)))
        orc = (ref.DiagQuadratic(d["q"], d["b"]), ref.NormL1(0.8), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(-1.0, 1.0)))
        return dev, orc, n, ny, 10.0 ** rng.uniform(-2, 0, ny), ys * rng.standard_normal(ny), xs * rng.standard_normal(n)
    return build


def sparse_ls(m, n, p=0.1, ys=1.0, xs=1.0, seed=0):
    """f(x) = 0.5 |Ax - b|^2 with A = structured / csr_of (oracle: LeastSquares of the dense matrix), c = Identity"""
    def build(bz, ref):
        A, (indptr, indices, data) = _structured_csr(m, n, p, seed)
        rng = _rng("ls-sparse-f", m, n, seed)
        b = rng.standard_normal(m)
        f = bz.SparseLeastSquares(indptr, indices, data, b, n)
        dev = (f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)))
        orc = (ref.LeastSquares(f.toarray(), b), ref.NormL1(0.1), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(-1.0, 1.0)))
        return dev, orc, n, n, 10.0 ** rng.uniform(-2, 0, n), ys * rng.standard_normal(n), xs * rng.standard_normal(n)
    return build


HEADLINE = ("diag", "l1", "box")

CASES = [
    Case("headline-1031-f64-M1", "headline", "float64", 1, family(1031, "float64", HEADLINE, "uni0", far=True), "f"),
    Case("headline-1031-f64-M2", "headline", "float64", 2, family(1031, "float64", HEADLINE, "uni0", far=True), "abc"),
    Case("headline-1031-f64-M3", "headline", "float64", 3, family(1031, "float64", HEADLINE, "uni1", far=True), "abc"),
    Case("headline-1031-f32-M1", "headline", "float32", 1, headline(1031, "float32", ys=1.0, xs=0.3, mu="elem", seed=0), "ef"),
    Case("headline-1031-f32-M2", "headline", "float32", 2, headline(1031, "float32", ys=3.0, xs=3.0, mu="uni", seed=5), "abc"),
    Case("headline-1031-f32-M3", "headline", "float32", 3, headline(1031, "float32", ys=3.0, xs=3.0, mu="uni", seed=5), "", free=True),
    Case("headline-2121-f64-M1", "headline", "float64", 1, family(2121, "float64", HEADLINE, "uni0", far=True), "e"),
    Case("headline-2121-f64-M1-b", "headline", "float64", 1, family(2121, "float64", HEADLINE, "uni1", far=True), "f"),
    Case("headline-2121-f64-M2", "headline", "float64", 2, family(2121, "float64", HEADLINE, "uni1", far=True), "abc"),
    Case("headline-2121-f64-M3", "headline", "float64", 3, headline(2121, "float64", ys=5.0, xs=3.0, mu="uni", seed=0), "abc"),
    Case("headline-2121-f32-M1", "headline", "float32", 1, headline(2121, "float32", ys=1.0, xs=0.3, mu="elem", seed=0), "ef"),
    Case("headline-2121-f32-M2", "headline", "float32", 2, family(2121, "float32", HEADLINE, "uni0", far=True), "abc"),
    Case("headline-2121-f32-M3", "headline", "float32", 3, family(2121, "float32", HEADLINE, "uni0", far=True), "", free=True),
    Case("diag-l1-cc-f32-M1", "family", "float32", 1, family(2202, "float32", ("diag", "l1", "cc"), "uni0", far=True), "f"),
    Case("diag-l1-cc-f32-M2", "family", "float32", 2, family(2202, "float32", ("diag", "l1", "cc"), "uni0", far=True), "abcde"),
    Case("diag-l1-cc-f32-M3", "family", "float32", 3, family(2202, "float32", ("diag", "l1", "cc"), "uni0", far=True), "abcde"),
    Case("diag-l1box-cc-n1030-M1", "family1030", "float64", 1, family(1030, "float64", ("diag", "l1box", "cc"), "uni0", far=True), "ef"),
    Case("diag-l1box-cc-n1030-M2", "family1030", "float64", 2, family(1030, "float64", ("diag", "l1box", "cc"), "uni0", far=True), "abcde"),
    Case("diag-l1box-cc-n1030-M3", "family1030", "float64", 3, family(1030, "float64", ("diag", "l1box", "cc"), "uni0", far=True), "abcde"),
    Case("diag-indbox_vec-box_vec-n1030-M1", "family1030", "float64", 1, family(1030, "float64", ("diag", "indbox_vec", "box_vec"), "uni0", far=True), "ef"),
    Case("diag-indbox_vec-box_vec-n1030-M2", "family1030", "float64", 2, family(1030, "float64", ("diag", "indbox_vec", "box_vec"), "uni0", far=True), "abc"),
    Case("diag-indbox_vec-box_vec-n1030-M3", "family1030", "float64", 3, family(1030, "float64", ("diag", "indbox_vec", "box_vec"), "uni0", far=True), "bd"),
    Case("zero-indbox_vec-box_vec-f64-M1", "family", "float64", 1, family(2041, "float64", ("zero", "indbox_vec", "box_vec"), "uni0", far=True), "f"),
    Case("zero-indbox_vec-box_vec-f64-M2", "family", "float64", 2, family(2041, "float64", ("zero", "indbox_vec", "box_vec"), "uni0", far=True), "abc"),
    Case("zero-indbox_vec-box_vec-f64-M3", "family", "float64", 3, family(2041, "float64", ("zero", "indbox_vec", "box_vec"), "uni0", far=False), "ab"),
    Case("zero-l1box-box-f64-M1", "family", "float64", 1, family(2201, "float64", ("zero", "l1box", "box"), "uni0", far=True), "ef"),
    Case("zero-l1box-box-f64-M2", "family", "float64", 2, family(2201, "float64", ("zero", "l1box", "box"), "uni0", far=True), "abc"),
    Case("zero-l1box-box-f64-M2-b", "family", "float64", 2, family(2201, "float64", ("zero", "l1box", "box"), "uni0", far=False), "bde"),
    Case("zero-l1box-box-f64-M3", "family", "float64", 3, family(2201, "float64", ("zero", "l1box", "box"), "uni0", far=False), "bde"),
    Case("zero-l1box-box-f64-M3-b", "family", "float64", 3, family(20001, "float64", ("zero", "l1box", "box"), "uni0", far=False), "abc"),
    Case("zero-l1box-box-f32-M1", "family", "float32", 1, family(2203, "float32", ("zero", "l1box", "box"), "uni2", far=True), "f"),
    Case("zero-l1box-box-f32-M2", "family", "float32", 2, family(2203, "float32", ("zero", "l1box", "box"), "uni2", far=True), "abc"),
    Case("zero-l1box-box-f32-M3", "family", "float32", 3, family(2203, "float32", ("zero", "l1box", "box"), "uni2", far=True), "abc"),
    Case("slack-l1-box-f64-M1", "slack", "float64", 1, slack(1000, "float64", "l1", "box", "uni0", far=False), "ef", slack=True),
    Case("slack-l1-box-f64-M2", "slack", "float64", 2, slack(1000, "float64", "l1", "box", "uni0", far=False), "abc", slack=True),
    Case("slack-l1-box-f64-M3", "slack", "float64", 3, slack(1000, "float64", "l1", "box", "uni0", far=False, seed="c"), "abc", slack=True),
    Case("slack-l1-box-f32-M1", "slack", "float32", 1, slack(1000, "float32", "l1", "box", "uni0", far=False), "ef", slack=True),
    Case("slack-l1-box-f32-M2", "slack", "float32", 2, slack(1000, "float32", "l1", "box", "uni1", far=False), "abc", slack=True),
    Case("slack-l1-box-f32-M3", "slack", "float32", 3, slack(1000, "float32", "l1", "box", "uni0", far=False, seed="d"), "abc", slack=True),
    Case("stencil-l1-box-M1", "stencil", "float64", 1, stencil(33, 46, ("l1", "box"), "uni0", far=False), "ef"),
    Case("stencil-l1-box-M2", "stencil", "float64", 2, stencil(33, 46, ("l1", "box"), "uni0", far=True), "abc"),
    Case("stencil-l1-box-M3", "stencil", "float64", 3, stencil(33, 46, ("l1", "box"), "uni0", far=False), "bd"),
    Case("dense-64x512-f64-M1", "dense", "float64", 1, dense_c(64, 512, "float64", ys=0.1, xs=0.0, seed=0), "f"),
    Case("dense-64x512-f64-M2", "dense", "float64", 2, dense_c(64, 512, "float64", ys=0.1, xs=0.0, seed=0), "abc"),
    Case("dense-64x512-f64-M3", "dense", "float64", 3, dense_c(64, 512, "float64", ys=1.0, xs=0.0, seed=2), "abc"),
    Case("dense-64x512-f32-M1", "dense", "float32", 1, dense_c(64, 512, "float32", ys=0.1, xs=0.0, seed=0), "f"),
    Case("dense-64x512-f32-M2", "dense", "float32", 2, dense_c(64, 512, "float32", ys=0.1, xs=0.0, seed=0), "abc"),
    Case("dense-64x512-f32-M3", "dense", "float32", 3, dense_c(64, 512, "float32", ys=3.0, xs=0.0, seed=0), "abc"),
    Case("dense-257x1028-f64-M1", "dense", "float64", 1, dense_c(257, 1028, "float64", ys=0.5, xs=0.0, seed=2), "f"),
    Case("dense-257x1028-f64-M2", "dense", "float64", 2, dense_c(257, 1028, "float64", ys=0.5, xs=0.0, seed=2), "ab"),
    Case("dense-257x1028-f64-M3", "dense", "float64", 3, dense_c(257, 1028, "float64", ys=0.5, xs=0.0, seed=2), "", free=True),
    Case("dense-257x1028-f32-M1", "dense", "float32", 1, dense_c(257, 1028, "float32", ys=0.5, xs=0.0, seed=2), "f"),
    Case("dense-257x1028-f32-M2", "dense", "float32", 2, dense_c(257, 1028, "float32", ys=0.5, xs=0.0, seed=2), "ab"),
    Case("dense-257x1028-f32-M3", "dense", "float32", 3, dense_c(257, 1028, "float32", ys=0.5, xs=0.0, seed=2), "", free=True),
    Case("sparse-c-M1", "sparse_c", "float64", 1, sparse_c(41, 121, ys=0.2, xs=0.3, seed=3), "ef"),
    Case("sparse-ls-M1", "sparse_ls", "float64", 1, sparse_ls(41, 121, ys=0.2, xs=0.3, seed=0), "ef"),
    Case("sparse-c-M2", "sparse_c", "float64", 2, sparse_c(41, 121, ys=0.2, xs=0.3, seed=0), "abe"),
    Case("sparse-c-M2-b", "sparse_c", "float64", 2, sparse_c(41, 121, ys=1.0, xs=1.0, seed=3), "abc"),
    Case("sparse-ls-M2", "sparse_ls", "float64", 2, sparse_ls(41, 121, ys=0.2, xs=0.3, seed=0), "abce"),
    Case("sparse-c-M3", "sparse_c", "float64", 3, sparse_c(41, 121, ys=0.2, xs=0.3, seed=0), "ab"),
    Case("sparse-c-M3-b", "sparse_c", "float64", 3, sparse_c(41, 121, ys=0.2, xs=0.3, seed=3), "bd"),
    Case("sparse-ls-M3", "sparse_ls", "float64", 3, sparse_ls(41, 121, ys=0.2, xs=0.3, seed=0), "abce"),
    Case("sparse-ls-M3-b", "sparse_ls", "float64", 3, sparse_ls(41, 121, ys=0.2, xs=0.3, seed=2), "bd"),
    Case("anderson-M2", "anderson", "float64", 2, headline(1031, "float64", ys=1.0, xs=0.3, mu="elem", seed=0), "abce", direction="anderson"),
    Case("anderson-M3", "anderson", "float64", 3, headline(1031, "float64", ys=1.0, xs=0.3, mu="elem", seed=0), "abe", direction="anderson"),
    Case("broyden-M2", "broyden", "float64", 2, headline(1031, "float64", ys=1.0, xs=0.3, mu="elem", seed=0), "abce", direction="broyden"),
    Case("broyden-M3", "broyden", "float64", 3, headline(1031, "float64", ys=1.0, xs=0.3, mu="elem", seed=0), "abce", direction="broyden"),
    # the two runs of tests/test_gpu_family_table.py that exhaust twenty backtracks, at that table's sizes, through step 50
    Case("diag-l1-cc-f32-M20", "family", "float32", 20, family(20002, "float32", ("diag", "l1", "cc"), "uni0", far=True), "ae", free=True, states=51),
    Case("zero-indbox_vec-box_vec-f64-M20", "family", "float64", 20, family(20001, "float64", ("zero", "indbox_vec", "box_vec"), "uni0", far=True),
         "", free=True, states=51),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
# Where no start meets the anchor rule, and what was tried on the oracle alone.
FREE = {
    "headline-1031-f32-M3": "fp32, M = 3, headline family: of some 200 starts (the family table's far starts in both regimes, the headline "
                            "builder over seven scales of y and x0 and eight seeds) none keeps a tau = 0 step with eight settled states "
                            "behind it; the case that runs reaches no tau = 0 step in 40 states",
    "headline-2121-f32-M3": "as headline-1031-f32-M3",
    "dense-257x1028-f64-M3": "M = 3 on cfg 4 at 257 x 1028: no step ends at tau = 0 within 40 states from any of 72 starts (nine scales "
                             "of y and x0, eight seeds); the case that runs takes backtracks and no tau = 0 step",
    "dense-257x1028-f32-M3": "as dense-257x1028-f64-M3",
    "diag-l1-cc-f32-M20": "the limit of 20 is met at step 43, behind a halving in trial 20 of step 42; compared through state 44",
    "zero-indbox_vec-box_vec-f64-M20": "the oracle takes 30 halvings and never ends a step at tau = 0 in 50 steps; 35 states are compared, "
                                       "so the steps where the forms used to part (45 on) are held form against form only",
}
# (g) a skipped pair at a step that ends at tau = 0: among the cases above the oracle gives two, both in fp32 (diag, l1, cc):
# step 32 of diag-l1-cc-f32-M2 and step 27 of diag-l1-cc-f32-M3, inside the compared range.  Twelve seeds of each pairwise
# kind at n = 62 (the sizes where tests/test_directions_host.py found its two) gave none.  Recorded, not asserted.
SKIPPED_AT_TAU0 = {"diag-l1-cc-f32-M2": 32, "diag-l1-cc-f32-M3": 27}


def case_ids(cases):
    return [c.name for c in cases]


# ----------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", ["headline-1031-f64-M2", "diag-l1box-cc-n1030-M3", "slack-l1-box-f32-M1", "broyden-M2", "dense-64x512-f32-M2"])
def test_recording_iteration_is_the_oracle(bz, ref, name):
    """the restated step and `PANOCplusIteration.step` side by side: the same bits in x, z, res, gamma, tau and the counts"""
    case = CASE[name]
    dev, orc, n, ny, mu, y, x0 = case.build(bz, ref)
    sts = []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for cls in (RecordingIteration, ref.PANOCplusIteration):
            if case.slack:
                F, G = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), x0[:n]), ref.NonsmoothCostFunSlack(orc[1], orc[3], n, ny)
            else:
                F, G = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0), ref.NonsmoothCostFun(orc[1])
            it = cls(F, G, x0, minimum_gamma=float(np.finfo(case.dtype).eps), max_backtracks=case.M, directions=case.directions(ref))
            sts.append((it, it.init()))
        for k in range(case.states - 1):
            a, b = [it.step(st) for it, st in sts]
            for u, v in ((a.x, b.x), (a.z, b.z), (a.res, b.res)):
                assert np.array_equal(u, v, equal_nan=True), (name, k)
            assert (a.gamma, a.tau, a.n_backtracks, a.n_gamma_halvings) == (b.gamma, b.tau, b.n_backtracks, b.n_gamma_halvings), (name, k)


@pytest.mark.parametrize("case", CASES, ids=case_ids(CASES))
def test_oracle_alone_produces_the_claimed_events_inside_the_compared_range(bz, ref, case):
    p = pair_of(bz, ref, case)
    tau0 = [j for j, s in enumerate(p.o.steps, 1) if s.tau == 0.0 and case.M >= 2]
    print(f"{case.name}: compared {p.compared} of {case.states} states; anchor step {p.anchor()}; steps ending at tau = 0: {len(tau0)} "
          f"({sum(1 for j in tau0 if j < p.compared)} compared); backtracks {sum(s.nbt for s in p.o.steps)}, halvings "
          f"{sum(s.halvings for s in p.o.steps)} (+{p.o.start_halvings} at the start); events in range "
          + " ".join(f"{k}:{len(v)}" for k, v in p.events.items()))
    for c in case.claims:
        assert p.events[c], (case.name, c, p.events, p.compared)
    if case.free:
        assert case.name in FREE
        return
    # the anchor and eight states behind it are compared: step a leads to state a + 1
    a = p.anchor()
    assert a is not None and a + 1 + BEHIND <= p.compared, (case.name, a, p.compared)
    assert set(case.claims) & set("adef"), case.name      # (what the anchor is: a step that ends at tau = 0, or (e) / (f))


def test_free_cases_are_the_listed_ones():
    assert {c.name for c in CASES if c.free} == set(FREE)


def test_every_event_is_claimed_on_every_path_that_can_show_it():
    """(a), (b), (c) on every path; (d), (e), (f) on the element-wise, stencil and sparse paths — cfg 4 (f = Zero beside a
    dense c) takes its halvings at the start only in every start tried, so (d) and (e) are claimed elsewhere"""
    by_path = {}
    for c in CASES:
        by_path.setdefault(c.path, set()).update(c.claims)
    print({k: "".join(sorted(v)) for k, v in by_path.items()})
    for path, ev in by_path.items():
        assert set("ab") <= ev, (path, ev)
    for path in ("headline", "family", "family1030", "slack", "sparse_c", "sparse_ls"):
        assert set("abcef") <= by_path[path], (path, by_path[path])
    for path in ("family", "family1030", "stencil", "sparse_c", "sparse_ls"):
        assert "d" in by_path[path], (path, by_path[path])
    assert "f" in by_path["dense"] and "e" in by_path["anderson"] and "e" in by_path["broyden"]


def test_skipped_pairs_at_tau_zero_are_where_recorded(bz, ref):
    for name, step in SKIPPED_AT_TAU0.items():
        p = pair_of(bz, ref, CASE[name])
        print(name, p.events["g"])
        assert step in p.events["g"]


def test_events_of_on_hand_made_steps():
    """the definitions of the module docstring on steps written out by hand (M = 3)"""
    class S:
        def __init__(self, tau, nbt, halvings, trials, ys_pos=True):
            self.tau, self.nbt, self.halvings, self.trials, self.ys_pos = tau, nbt, halvings, trials, ys_pos
    t = lambda k, br, me=1.0: (k, -1.0, None if br == "halve" else me, 0.0, br)
    steps = [S(1.0, 0, 0, [t(1, "accept", -1.0)]),                                          # (b)
             S(0.0, 2, 0, [t(1, "reject"), t(2, "reject"), t(3, "accept")]),                # (a)
             S(0.0, 1, 1, [t(1, "halve"), t(2, "reject"), t(3, "accept")], ys_pos=False),   # (c), (d), (g): not (a), one backtrack
             S(0.5, 1, 1, [t(1, "reject"), t(2, "accept", -1.0)][:1] + [t(2, "halve"), t(3, "halve")]),      # (e), tau = 1/2
             S(0.0, 2, 1, [t(1, "reject"), t(2, "reject"), t(3, "halve")])]                 # (c)? no: the step before kept tau; (d), (e)
    ev = events_of(steps, 3)
    assert ev == {"a": [2], "b": [1], "c": [3], "d": [3, 5], "e": [4, 5], "f": [], "g": [3]}, ev
    assert events_of([S(1.0, 0, 0, [t(1, "accept", 2.0)]), S(1.0, 0, 1, [t(1, "halve")]), S(1.0, 0, 0, [t(1, "accept", -2.0)])], 1) == \
        {"a": [], "b": [], "c": [], "d": [], "e": [2], "f": [1], "g": []}


def test_settled_rule():
    eps = 2.0 ** -52
    class S:
        def __init__(self, trials, ys_pos=True):
            self.trials, self.ys_pos = trials, ys_pos
    a = S([(1, -1.0, 0.5, 3.0, "reject"), (2, -1.0, 7.0, 3.0, "accept")])
    assert settled(a, S([(1, -1.0, 0.5 + 1e-3, 3.0, "reject"), (2, -1.0, -7.0, 3.0, "accept")]), eps, 2)      # trial M: no decision
    assert not settled(a, S([(1, -1.0, 0.5 + 1e-2, 3.0, "reject"), (2, -1.0, 7.0, 3.0, "accept")]), eps, 2)   # 0.5 < 100 * 1e-2
    assert not settled(a, S(a.trials, ys_pos=False), eps, 2)
    assert not settled(a, S([(1, -1.0, -0.5, 3.0, "accept")]), eps, 2)
    b = S([(1, 30 * eps, 0.5, 3.0, "halve")])
    assert not settled(b, b, eps, 2)                                                                          # under the floor
    assert settled(S([(1, 50 * eps, None, 3.0, "halve")]), S([(1, 50 * eps, None, 3.0, "halve")]), eps, 2)
