"""`directions` other than L-BFGS, the part that needs no GPU: the oracle twin of the device's Anderson arithmetic, the
table of cases that tests/test_gpu_directions_table.py runs on the device, and the proof that the oracle alone produces
the events each case claims.

The restatement (`_AndersonOperator` of oracle/bazinga_ref.py) solves min |Y a - v| by a QR least squares; the device
solves the normal equations (Y'Y) a = Y'v from the Gram products its passes return (LbfgsMemory::anderson_coefficients,
bz_lbfgs_host.h).  The two agree to cond(Y)^2 eps, which is what the 1e-6 of tests/test_gpu_directions.py pays for.
`AndersonTwin` is the restatement with the coefficients formed as the device forms them — Gram products through the
oracle's `_dot` (so a reducer applies), float64 elimination with complete pivoting and the 1e-14 relative pivot cut-off —
and is pinned from both sides here: bit for bit to the header, and to the lstsq restatement within the conditioning.

The oracle has no keyword for the operator, but `PANOCplusIteration.init()` returns a state whose `H` is the operator and
never touches it: `OracleRun` replaces `st.H` there.  `BroydenProbe` is `_BroydenOperator` itself plus a record of which
branch of theta each update took (the arithmetic is the base class's)."""
import zlib

import numpy as np
import pytest

from oracle import bazinga_ref as REF
from tests.test_lbfgs_host import _anderson, driver      # noqa: F401  (the stand-alone driver of the host header)

CM = 5
BLOCK = 256          # bz_kernels.h
PIVOT_CUT = 1e-14


# ------------------------------------------------------------------------------------------------- the Anderson twin
def gram_solve(G, w):
    """a = G^-1 w in float64 by elimination with complete pivoting; a pivot not above 1e-14 of the largest diagonal entry
    ends it (rank deficiency: the remaining coefficients are zero) — the loops of LbfgsMemory::anderson_coefficients"""
    m = len(w)
    A = [[float(G[i][j]) for j in range(m)] for i in range(m)]
    b = [float(v) for v in w]
    perm = list(range(m))
    amax = 0.0
    for i in range(m):
        amax = max(amax, abs(A[i][i]))
    rank = 0
    for k in range(m):
        pi, pj, best = k, k, 0.0
        for i in range(k, m):
            for j in range(k, m):
                if abs(A[i][j]) > best:
                    best, pi, pj = abs(A[i][j]), i, j
        if not best > PIVOT_CUT * amax:
            break
        if pi != k:
            A[k], A[pi] = A[pi], A[k]
            b[k], b[pi] = b[pi], b[k]
        if pj != k:
            for i in range(m):
                A[i][k], A[i][pj] = A[i][pj], A[i][k]
            perm[k], perm[pj] = perm[pj], perm[k]
        for i in range(k + 1, m):
            f = A[i][k] / A[k][k]
            for j in range(k, m):
                A[i][j] -= f * A[k][j]
            b[i] -= f * b[k]
        rank = k + 1
    z = [0.0] * m
    for k in range(rank - 1, -1, -1):
        acc = b[k]
        for j in range(k + 1, rank):
            acc -= A[k][j] * z[j]
        z[k] = acc / A[k][k]
    a = np.zeros(m)
    for k in range(rank):
        a[perm[k]] = z[k]
    return a


class AndersonTwin(REF._AndersonOperator):
    """`_AndersonOperator` with a = (Y'Y)^-1 Y'v formed as on the device.  The Gram matrix grows by one row per stored
    pair (its products with the pairs already stored, taken when it arrives) and loses its oldest row when the ring is
    full, as LbfgsMemory::gram_insert keeps it.  `log` receives (a, a_lstsq, cond(Y), |Y|, |v|) of every application."""

    def __init__(self, M, x, log=None):
        super().__init__(M, x)
        self.G = np.zeros((0, 0))
        self.log = log

    def update(self, s, y):
        yy = [float(REF._dot(yi, y)) for yi in self.Y]
        G = self.G
        if len(self.Y) == self.M:
            G, yy = G[1:, 1:], yy[1:]
        m = len(yy)
        Gn = np.zeros((m + 1, m + 1))
        Gn[:m, :m] = G
        Gn[:m, m] = Gn[m, :m] = yy
        Gn[m, m] = float(REF._dot(y, y))
        self.G = Gn
        return super().update(s, y)

    def reset(self):
        super().reset()
        self.G = np.zeros((0, 0))

    def mul(self, d, v):
        d[...] = v
        if self.S:
            w = [float(REF._dot(yi, v)) for yi in self.Y]
            a = gram_solve(self.G, w)
            Ym, Sm = np.stack(self.Y, axis=1), np.stack(self.S, axis=1)
            if self.log is not None:
                Y64 = Ym.astype(np.float64)
                sv = np.linalg.svd(Y64, compute_uv=False)
                self.log.append((a, np.linalg.lstsq(Y64, v.astype(np.float64), rcond=None)[0], float(sv[0] / sv[-1]),
                                 float(sv[0]), float(np.linalg.norm(v.astype(np.float64)))))
            d += (Sm - Ym) @ a.astype(v.dtype)
        return d


class BroydenProbe(REF._BroydenOperator):
    """the oracle's operator; `branches` receives, per update, which way it went: "ss0" (the early return on <s, s> <= 0),
    "big" (|delta| >= theta_bar), "pos" (0 <= delta < theta_bar), "neg" (-theta_bar < delta < 0), "denom0\""""

    def __init__(self, theta_bar, x, branches=None):
        super().__init__(theta_bar, x)
        self.branches = branches if branches is not None else []

    def update(self, s, y):
        T = s.dtype.type
        ss, hys = REF._dot(s, s), REF._dot(self.Hm @ y, s)
        if not ss > 0:
            self.branches.append("ss0")
        else:
            delta = hys / ss
            tag = "big" if not abs(delta) < self.theta_bar else ("pos" if delta >= 0 else "neg")
            theta = T(1) if tag == "big" else (T(1) - (T(1) if delta >= 0 else T(-1)) * self.theta_bar) / (T(1) - delta)
            denom = (T(1) / theta - T(1)) * ss + hys
            self.branches.append("denom0" if denom == 0 or denom != denom else tag)
        return super().update(s, y)


# ------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One run of the table.  kind: "anderson" (param = memory) or "broyden" (param = theta_bar); build(bz, ref) ->
    (dev oracles, ref oracles, n, ny, mu, y, x0); kw: step-size keywords of both solvers (gamma, adaptive); slack: the
    lifted form of ALS; claims: events the run must contain — "halving" (a gamma halving inside a step, not at the start),
    "backtrack" (a tau backtrack), "nonpos" (a kept pair with <s, y> <= 0), "big" / "pos" / "neg" / "ss0" (theta branches)."""

    def __init__(self, name, kind, param, dt, iters, build, claims=(), kw=None, fuse=True, slack=False):
        self.name, self.kind, self.param, self.dtype, self.iters = name, kind, param, np.dtype(dt).type, iters
        self.build, self.claims, self.kw, self.fuse, self.slack = build, tuple(claims), dict(kw or {}), fuse, slack

    def __repr__(self):
        return self.name

    def directions(self, m):
        """the `directions` object of module m (the package or the oracle)"""
        return m.AndersonAcceleration(self.param) if self.kind == "anderson" else m.Broyden(theta_bar=self.param)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def headline(n, dt, ys=0.2, xs=0.0, mu="uni", seed=0):
    """the headline family (DiagQuadratic, NormL1, Box), c = Identity"""
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg2
        dtype = np.dtype(dt).type
        d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
        rng = _rng("headline", n, dt, seed)
        mu_ = np.full(n, 0.1, dtype) if mu == "uni" else (10.0 ** rng.uniform(-2, 0, n)).astype(dtype)
        return dev, orc, n, n, mu_, (ys * rng.standard_normal(n)).astype(dtype), (xs * rng.standard_normal(n)).astype(dtype)
    return build


def cfg2(n, dt, g, ys=0.2, xs=0.0, seed=0):
    """make_cfg2 with another g (an Lp kind: the kernel chain)"""
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg2
        dtype = np.dtype(dt).type
        d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype, g=g)
        rng = _rng("cfg2", g, n, dt, seed)
        return dev, orc, n, n, np.full(n, 0.1, dtype), (ys * rng.standard_normal(n)).astype(dtype), \
            (xs * rng.standard_normal(n)).astype(dtype)
    return build


def family(n, dt, fam, regime="uni0", far=False):
    """a family of the one-pass table with its vector bounds and per-element penalties (tests/test_gpu_family_table.py)"""
    def build(bz, ref):
        from tests.test_gpu_family_table import make_case
        dev, orc, mu, y, x0 = make_case(bz, ref, n, fam, np.dtype(dt).type, regime, far=far)
        return dev, orc, n, n, mu, y, x0
    return build


def group_l21(n, dt, K=3):
    def build(bz, ref):
        dtype = np.dtype(dt).type
        d = bz.synth.l1_quadratic(n, dtype=dtype)
        g = bz.NormL21(2.5, K)          # (the package's own host prox is the oracle of this g: tests/test_gpu_group_lasso.py)
        box = bz.ClosedSet(bz.IndBox(-1.0, 1.0)), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1)))
        rng = _rng("l21", n, dt)
        return (bz.DiagQuadratic(d["q"], d["b"]), g, bz.IdentityFunction(), box[0]), \
            (ref.DiagQuadratic(d["q"], d["b"]), g, ref.IdentityFunction(), box[1]), n, n, np.full(n, 0.1, dtype), \
            (0.2 * rng.standard_normal(n)).astype(dtype), np.zeros(n, dtype)
    return build


def weighted_l1(n, dt):
    """NormL1 with a per-element lambda (zeros included) beside DiagQuadratic and a box D"""
    def build(bz, ref):
        dtype = np.dtype(dt).type
        d = bz.synth.l1_quadratic(n, dtype=dtype)
        rng = _rng("wl1", n, dt)
        lam = np.where(np.arange(n) % 7 == 0, 0.0, rng.uniform(0.5, 4.0, n)).astype(dtype)
        return (bz.DiagQuadratic(d["q"], d["b"]), bz.NormL1(lam), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0))), \
            (ref.DiagQuadratic(d["q"], d["b"]), ref.NormL1(lam), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1)))), \
            n, n, np.full(n, 0.1, dtype), (0.2 * rng.standard_normal(n)).astype(dtype), np.zeros(n, dtype)
    return build


def stencil(nx, ny_):
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg3
        d, n, dev, orc = make_cfg3(bz, ref, nx, ny_, load=-1.0)
        return dev, orc, n, n, np.full(n, 0.1), np.zeros(n), d["x0"]
    return build


def dense_c(ny, n, dt):
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg4
        dtype = np.dtype(dt).type
        d, dev, orc = make_cfg4(bz, ref, ny, n, dtype)
        rng = _rng("dense", ny, n, dt)
        return dev, orc, n, ny, np.full(ny, 0.1, dtype), (0.1 * rng.standard_normal(ny)).astype(dtype), np.zeros(n, dtype)
    return build


def sparse_c(n, m):
    def build(bz, ref):
        from tests.test_gpu_sparse import CsrOracle
        d = bz.synth.budget_bands(n, m)
        csr = (d["indptr"], d["indices"], d["data"], d["b"], n)
        dev = (bz.DiagQuadratic(d["q"], d["fb"]), bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
        orc = (ref.DiagQuadratic(d["q"], d["fb"]), ref.IndBox(0.0, 1.0), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(d["lo"], d["hi"])))
        rng = _rng("sparse", n, m)
        # (mu = 1: with mu = 0.1 from x0 = 0 the first six steps take 34 tau backtracks, cond(Y) reaches 1e4 and the oracle's
        # own two roundings part by 6e-11 within 14 states)
        return dev, orc, n, m + 1, np.full(m + 1, 1.0), 0.1 * rng.standard_normal(m + 1), np.zeros(n)
    return build


def pairs(n, kind, g="l1", xs=0.3, seed=0):
    def build(bz, ref):
        from tests.test_gpu_parity import make_pairs
        dev, orc = make_pairs(bz, ref, n, kind, g=g)
        rng = _rng("pairs", n, kind, seed)
        return dev, orc, n, n, 10.0 ** rng.uniform(-2, 0, n), rng.standard_normal(n), xs * rng.standard_normal(n)
    return build


def slack_headline(n, dt):
    """the lifted vector [x; s] of ALS on the headline problem (tests/test_gpu_als.py)"""
    def build(bz, ref):
        from tests.test_gpu_parity import make_cfg2
        dtype = np.dtype(dt).type
        d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
        rng = _rng("slack", n, dt)
        mu, y = np.full(n, 0.1, dtype), rng.standard_normal(n).astype(dtype)
        return dev, orc, n, n, mu, y, np.concatenate([np.zeros(n), np.clip(rng.standard_normal(n), -1, 1)]).astype(dtype)
    return build


def zero_f(n, dt):
    """f = Zero with multipliers small enough that c(x) + mu*y stays in D and a start inside D but for one element (which
    keeps the smoothness estimate finite): the subproblem is min g(x), solved at 0 within a few iterations, after which
    s = 0 exactly (the notes on f = Zero in tests/test_gpu_family_table.py)"""
    def build(bz, ref):
        dtype = np.dtype(dt).type
        rng = _rng("zerof", n, dt)
        dev = (bz.Zero(), bz.NormL1(0.8), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)))
        orc = (ref.Zero(), ref.NormL1(dtype(0.8)), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1))))
        x0 = (0.02 * rng.standard_normal(n)).astype(dtype)
        x0[0] = 1.5
        return dev, orc, n, n, np.full(n, 0.1, dtype), (0.5 * rng.standard_normal(n)).astype(dtype), x0
    return build


HALVE = dict(gamma=2.0, adaptive=True)      # far above 0.95 / L: the start halves it, and so do later steps (per-element mu)

ANDERSON_CASES = [
    # the headline family in its default form, every memory, both types, last pack ragged
    # (from x0 = 0 with small multipliers this problem asks for a gamma halving in its first steps and, with a memory of
    # two or more, for tau backtracks: the tau-backtracked passes take the TRIAL instantiation)
    Case("headline-m1-f64", "anderson", 1, "float64", 14, headline(4001, "float64"), ["halving"]),
    Case("headline-m2-f64", "anderson", 2, "float64", 14, headline(4001, "float64"), ["halving", "backtrack"]),
    Case("headline-m3-f64", "anderson", 3, "float64", 14, headline(4001, "float64"), ["halving", "backtrack"]),
    Case("headline-m5-f64", "anderson", 5, "float64", 14, headline(4001, "float64"), ["halving", "backtrack"]),
    Case("headline-m1-f32", "anderson", 1, "float32", 14, headline(4003, "float32"), ["halving"]),
    Case("headline-m2-f32", "anderson", 2, "float32", 14, headline(4003, "float32"), ["halving", "backtrack"]),
    Case("headline-m3-f32", "anderson", 3, "float32", 14, headline(4003, "float32"), ["halving", "backtrack"]),
    Case("headline-m5-f32", "anderson", 5, "float32", 14, headline(4003, "float32"), ["halving", "backtrack"]),
    # a family of the table: vector bounds on both g and D, per-element penalties (UNI = 0)
    Case("indboxvec-boxvec-m5-f64", "anderson", 5, "float64", 14, family(2001, "float64", ("diag", "indbox_vec", "box_vec"))),
    Case("indboxvec-boxvec-m2-f32", "anderson", 2, "float32", 14, family(2003, "float32", ("diag", "indbox_vec", "box_vec"))),
    # a nonconvex pairwise D: pairs with <s, y> <= 0 are kept.  (Rare: of some 500 seeded runs of 16 states over
    # xor / vc / cc / eitheror at n = 62 .. 2002, these two had one without a storm of halvings; none at n = 2002.)
    Case("l1-vc-n62-m3-f64", "anderson", 3, "float64", 16, pairs(62, "vc", xs=3.0, seed=1), ["nonpos"]),
    Case("zero-vc-n502-m3-f64", "anderson", 3, "float64", 18, pairs(502, "vc", g="zero", xs=1.0, seed=5), ["nonpos", "halving"]),
    Case("l1-xor-m5-f64", "anderson", 5, "float64", 16, family(2002, "float64", ("diag", "l1", "xor"), far=True)),
    Case("l1-xor-m3-f32", "anderson", 3, "float32", 16, family(2002, "float32", ("diag", "l1", "xor"), far=True), ["backtrack"]),
    # the kernel chain (k_compact_xd)
    Case("chain-m2-f64", "anderson", 2, "float64", 14, headline(4001, "float64"), fuse=False),
    Case("chain-m5-f32", "anderson", 5, "float32", 14, headline(4003, "float32"), fuse=False),
    # stencil f on a ragged grid (rows of whole 16-byte packs: the library refuses 47 columns)
    Case("stencil-33x46-m3", "anderson", 3, "float64", 14, stencil(33, 46)),
    # dense and sparse c
    Case("dense-20x100-m5-f64", "anderson", 5, "float64", 14, dense_c(20, 100, "float64")),
    Case("dense-20x100-m2-f32", "anderson", 2, "float32", 14, dense_c(20, 100, "float32")),
    Case("dense-64x512-m3-f64", "anderson", 3, "float64", 14, dense_c(64, 512, "float64")),
    Case("dense-64x512-m5-f32", "anderson", 5, "float32", 14, dense_c(64, 512, "float32")),
    Case("sparse-300x100-m3", "anderson", 3, "float64", 14, sparse_c(300, 100), ["backtrack"]),
    # group and Lp kinds of g (kernel chain)
    Case("l21-m3-f64", "anderson", 3, "float64", 14, group_l21(2001, "float64")),
    Case("lpnonneg-m2-f64", "anderson", 2, "float64", 14, cfg2(2001, "float64", "lpnonneg")),
    Case("wl1-m3-f64", "anderson", 3, "float64", 14, weighted_l1(2001, "float64")),
    # the slack form of ALS
    Case("slack-m3-f64", "anderson", 3, "float64", 14, slack_headline(1000, "float64"), slack=True),
    # a gamma halving in mid-run
    Case("halving-m3-f64", "anderson", 3, "float64", 16, headline(4001, "float64", ys=1.0, xs=0.3, mu="elem"), ["halving"], kw=HALVE),
]

BROYDEN_CASES = [
    Case("n2-f64", "broyden", 0.2, "float64", 8, headline(2, "float64", xs=0.5)),
    Case("n63-f64-t02", "broyden", 0.2, "float64", 16, headline(63, "float64")),
    Case("n63-f32-t09", "broyden", 0.9, "float32", 16, headline(63, "float32"), ["pos"]),
    Case("n1024-f32", "broyden", 0.2, "float32", 12, headline(1024, "float32")),
    Case("n1030-f64", "broyden", 0.9, "float64", 12, headline(1030, "float64")),
    Case("n1030-f32", "broyden", 0.2, "float32", 12, headline(1030, "float32")),
    Case("n1031-f64", "broyden", 0.2, "float64", 12, headline(1031, "float64")),
    Case("n4096-f64", "broyden", 0.2, "float64", 6, headline(4096, "float64")),
    Case("n4096-f32", "broyden", 0.9, "float32", 6, headline(4096, "float32")),
    Case("zero-s-n63", "broyden", 0.2, "float64", 12, zero_f(63, "float64"), ["ss0", "backtrack"]),
    Case("halving-n63", "broyden", 0.2, "float64", 16, headline(63, "float64", ys=1.0, xs=1.0, mu="elem"), ["halving"], kw=HALVE),
    Case("backtrack-n63", "broyden", 0.2, "float64", 16, headline(63, "float64", ys=5.0, xs=3.0, mu="elem"), ["backtrack", "neg"]),
    Case("dense-20x100", "broyden", 0.2, "float64", 14, dense_c(20, 100, "float64")),
    # (s'H borrows the dense-constraint kernels with f forced to Zero: nothing else of the element parameters may leak in)
    Case("wl1-n63", "broyden", 0.2, "float64", 14, weighted_l1(63, "float64")),
    Case("l21-n63", "broyden", 0.9, "float64", 14, group_l21(63, "float64")),
    Case("xor-n62", "broyden", 0.2, "float64", 16, pairs(62, "xor"), ["neg", "big", "pos", "halving", "backtrack"]),
]
# the theta branches that must occur somewhere in the Broyden table
THETA_BRANCHES = ("big", "pos", "neg")

CASES = {c.name: c for c in ANDERSON_CASES + BROYDEN_CASES}
assert len(CASES) == len(ANDERSON_CASES) + len(BROYDEN_CASES)


def case_ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ the oracle's side
class OracleRun:
    """The oracle's iteration of a case, with the twin (Anderson) or the probe (Broyden) as its operator, under a reducer
    of the caller's.  `events` counts what the steps did; `log` / `branches` are the operator's own records."""

    def __init__(self, ref, case, built, reducer=None):
        dev, orc, n, ny, mu, y, x0 = built
        self.ref, self.reducer, self.case = ref, reducer, case
        self.log, self.branches, self.steps = [], [], []      # (steps: halvings, backtracks, <s, y> <= 0 of every step)
        self.events = {"halving": 0, "start_halvings": 0, "backtrack": 0, "nonpos": 0}
        ref.set_reducer(reducer)
        try:
            if case.slack:
                F = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), x0[:n])
                G = ref.NonsmoothCostFunSlack(orc[1], orc[3], n, ny)
            else:
                F, G = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0), ref.NonsmoothCostFun(orc[1])
            self.it = ref.PANOCplusIteration(F, G, x0, minimum_gamma=float(np.finfo(case.dtype).eps),
                                             directions=case.directions(ref), **case.kw)
            self.st = self.it.init()
            if case.kind == "broyden":
                self.st.H = BroydenProbe(case.param, self.st.x, self.branches)
            else:
                self.st.H = AndersonTwin(case.param, self.st.x, self.log)
            self.events["start_halvings"] = self.st.n_gamma_halvings
        finally:
            ref.set_reducer(None)

    def step(self):
        self.ref.set_reducer(self.reducer)
        try:
            h0 = self.st.n_gamma_halvings
            self.st = self.it.step(self.st)
        finally:
            self.ref.set_reducer(None)
        self.events["halving"] += self.st.n_gamma_halvings - h0
        self.events["backtrack"] += self.st.n_backtracks
        self.events["nonpos"] += int(not self.st.last_ys > 0)
        self.steps.append((self.st.n_gamma_halvings - h0, self.st.n_backtracks, bool(not self.st.last_ys > 0)))
        return self.st

    def counts(self):
        out = dict(self.events)
        for b in ("ss0", "big", "pos", "neg", "denom0"):
            out[b] = self.branches.count(b)
        return out


_EVENTS = {}


def oracle_events(bz, ref, case):
    """the events of a case on the oracle alone (computed once per session), with the twin-vs-lstsq records of Anderson"""
    if case.name not in _EVENTS:
        with np.errstate(all="ignore"):
            run = OracleRun(ref, case, case.build(bz, ref))
            for _ in range(case.iters - 1):
                run.step()
        _EVENTS[case.name] = (run.counts(), run.log)
    return _EVENTS[case.name]


def plan_chunks(rows, cols, packn):
    """Solver::plan_chunks: rows per chunk and chunks of the transposed product's row-chunk partials"""
    colblocks = max(1, (cols // packn + BLOCK - 1) // BLOCK)
    chunks = max(1, min(rows, (2048 + colblocks - 1) // colblocks))
    rpc = (rows + chunks - 1) // chunks
    return rpc, (rows + rpc - 1) // rpc


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_twin_coefficients_equal_the_header_bit_for_bit(driver, m):
    """random full-rank Gram systems: the twin's elimination and LbfgsMemory::anderson_coefficients give the same bits"""
    for trial in range(6):
        rng = np.random.default_rng(1000 * m + trial)
        Y = rng.standard_normal((m, 8)) * 10.0 ** rng.uniform(-3, 3, (m, 1))
        w = Y @ rng.standard_normal(8)
        a, G = _anderson(driver, Y, w)
        assert np.array_equal(gram_solve(G, w), a), (m, trial)


def test_twin_treats_a_rank_deficiency_as_the_header_does(driver):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((4, 8))
    Y[3] = Y[1]
    w = Y @ rng.standard_normal(8)
    a, G = _anderson(driver, Y, w)
    assert np.array_equal(gram_solve(G, w), a) and np.count_nonzero(a == 0.0) == 1


@pytest.mark.parametrize("case", ANDERSON_CASES, ids=case_ids(ANDERSON_CASES))
def test_twin_is_the_lstsq_restatement_within_the_conditioning(bz, ref, case):
    """Every application of every Anderson case: the twin's coefficients against the lstsq restatement's, cond(Y) of the
    oracle's own Y at that state.  The bound is cond(Y)^2 eps with the two constants the bare product leaves out:
      - the Gram products are rounded sums of n rounded products: u = (ceil(log2 n) + 1 + m) eps, the depth of a pairwise sum
        and the m elimination steps, eps of the type the products are rounded to;
      - Y'v cancels where v is far from the span of Y: G a = w with |dG| <= u |Y|^2 and |dw| <= u |Y| |v| gives
        |da| / |a| <= cond(Y)^2 u (1 + |v| / (|Y| |a|))      (2-norms; the sensitivity of a least-squares problem with a
        large residual, Golub & Van Loan 5.3.7).
    With cond(Y) = 1 (memory 1) the bare cond(Y)^2 eps would ask one division of two rounded 4001-term sums to be exact to
    one unit: measured there 4.4 eps.  Measured worst |da| / (cond(Y)^2 eps |a|) over the table: 23 (indboxvec-boxvec-m5-
    f64, cond(Y) = 15); worst ratio to the bound below (printed): 0.09."""
    counts, log = oracle_events(bz, ref, case)
    eps = float(np.finfo(case.dtype).eps)
    n = len(case.build(bz, ref)[6])
    assert len(log) >= case.iters - 4       # (an application per step but the first, and the first after each reset)
    worst = bare = 0.0
    for a, a_ls, cond, ynorm, vnorm in log:
        u = (int(np.ceil(np.log2(n))) + 1 + len(a)) * eps
        da, na = float(np.linalg.norm(a - a_ls)), float(np.linalg.norm(a_ls))
        worst = max(worst, da / (cond ** 2 * u * (na + vnorm / ynorm)))
        bare = max(bare, da / (cond ** 2 * eps * na))
    print(f"{case.name}: largest |a_twin - a_lstsq| / bound = {worst:.3e}, / (cond(Y)^2 eps |a_lstsq|) = {bare:.3e}, "
          f"largest cond(Y) = {max(r[2] for r in log):.3e}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case", ANDERSON_CASES + BROYDEN_CASES, ids=case_ids(ANDERSON_CASES + BROYDEN_CASES))
def test_oracle_alone_produces_the_claimed_events(bz, ref, case):
    counts, _ = oracle_events(bz, ref, case)
    print(case.name, counts)
    for claim in case.claims:
        assert counts[claim] >= 1, (case.name, claim, counts)
    if case.kind == "broyden":
        assert counts["denom0"] == 0
        if "ss0" not in case.claims:       # (an update per step, none of them the early return)
            assert counts["ss0"] == 0 and counts["big"] + counts["pos"] + counts["neg"] == case.iters - 1


def test_every_theta_branch_occurs_in_the_broyden_table(bz, ref):
    total = {b: 0 for b in THETA_BRANCHES}
    for case in BROYDEN_CASES:
        counts, _ = oracle_events(bz, ref, case)
        for b in THETA_BRANCHES:
            total[b] += counts[b]
    print(total)
    assert all(total[b] >= 1 for b in THETA_BRANCHES), total
    # ... and with both values of theta_bar
    assert {c.param for c in BROYDEN_CASES} == {0.2, 0.9}


def test_broyden_sizes_reach_the_chunk_plans_they_are_chosen_for():
    """n x n operator, the transposed product's plan (Solver::plan_chunks, gemv_cols): fp64 packs hold 2, fp32 packs 4"""
    assert plan_chunks(600, 600, 2) == (1, 600)                  # (the size of tests/test_gpu_directions.py: a row per chunk)
    assert plan_chunks(2, 2, 2) == (1, 2) and plan_chunks(63, 63, 2) == (1, 63) and plan_chunks(63, 63, 4) == (1, 63)
    assert plan_chunks(1024, 1024, 4) == (1, 1024) and 1024 % 64 == 0            # MFMA, a row per chunk
    assert plan_chunks(1030, 1030, 2) == (2, 515) and plan_chunks(1030, 1030, 4) == (2, 515)      # two rows, last chunk full
    assert 1030 % 4 == 2 and 1030 % 2 == 0 and 1030 % 64 != 0    # unaligned columns in fp32, aligned in fp64, VALU in both
    assert plan_chunks(1031, 1031, 2) == (2, 516) and 1031 - 2 * 515 == 1         # two rows, a ragged last chunk of one
    assert plan_chunks(4096, 4096, 2) == (16, 256) and plan_chunks(4096, 4096, 4) == (8, 512) and 4096 % 64 == 0


def test_broyden_operator_after_a_halving_is_the_identity_plus_that_steps_update(bz, ref):
    """A gamma halving resets the operator to the identity INSIDE the step; the step still ends with update!(H, s, y).  So
    the first direction after a halving is not -res: the operator is the identity plus one rank-one term (and the device
    does the same: broyden_reset in lbfgs_reset, broyden_update in commit)."""
    case = CASES["halving-n63"]
    run = OracleRun(ref, case, case.build(bz, ref))
    seen = 0
    for _ in range(case.iters - 1):
        run.step()
        if run.steps[-1][0]:
            E = run.st.H.Hm - np.eye(run.st.H.n)
            assert np.linalg.matrix_rank(E) == 1 and run.branches[-1] in THETA_BRANCHES
            seen += 1
        elif seen:
            assert np.linalg.matrix_rank(run.st.H.Hm - np.eye(run.st.H.n)) >= 2      # (... and grows from there)
            break
    assert seen >= 1
