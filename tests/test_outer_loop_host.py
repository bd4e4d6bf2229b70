"""The inputs of tests/test_gpu_outer_loop.py and their preconditions, checked on the oracle alone (no GPU): a device run
cannot pass that file by vacuity.

The outer loops of alps / als are compared with the oracle bit for bit.  What makes that possible: the subsolver is
PANOCplus(maxit=1, gamma=GAMMA, adaptive=False) on both sides — the initial state's z = prox_{gamma g}(x - gamma grad L(x)),
no Lipschitz estimate, no step-size test — with c = Identity and an element-wise f.  Then x, y, s and mu after every outer
iteration are element-wise functions of the inputs, norm_res_prim is a maximum, inner_tol and the theta test are a few
double operations, and default_penalty_parameter! depends on a reduced value only through max(1, objx): the generator
keeps f(x) + g(x) <= 1 at the start, so that denominator is exactly 1.

f = Zero appears only beside g in {zero, indbox, indbox_vec}, whose value is 0: with any other g the start's objective
lambda * |x|_1 (or lambda * nnz) exceeds 1 as soon as an entry is far from D, and the denominator would be a sum."""
import warnings
import zlib

import numpy as np
import pytest

G_KINDS = ("zero", "l1", "nonneg", "l1box", "l0box", "indbox", "indbox_vec")
D_KINDS = ("zero", "free", "box", "box_vec", "vc", "cc", "eitheror", "xor")
SLACK_D_KINDS = ("zero", "free", "box", "box_vec")
PAIRWISE = ("vc", "cc", "eitheror", "xor")
TYPES = ("float64", "float32")
REGIMES = ("uni0", "uni1", "uni2", "last")
VEC_FORMS = ("both", "lo_vec_hi_inf", "lo_num_hi_vec")
NONNEG_G = ("nonneg", "l1box", "l0box")          # prox_g(x) >= 0
ZERO_VALUED_G = ("zero", "indbox", "indbox_vec")
K_OUTER = 6
GAMMA = 0.02
G_LO, G_HI = -2.5, 3.0          # g = IndBox with scalar bounds: wide enough that a clipped entry can still be far from D
D_LO, D_HI = -0.5, 0.7          # D = Box with scalar bounds


def pack_of(dtype):
    return 16 // np.dtype(dtype).itemsize


def cannot_be_far(g, D):
    """classes where no x = prox_g(x0) is further than sqrt(2) from D: mu is uniform whatever the regime asks for"""
    return D == "free" or (g in NONNEG_G and D in ("vc", "eitheror"))


def pair_at_distance(D, d, dform, dlo, dhi, i):
    """two adjacent arguments (elements i, i + 1) of which at least one lies at distance d from D (a pair set: from the
    pair's projection).  dlo / dhi: the vector bounds of D = box_vec."""
    if D in ("zero", "free"):
        return d, -d - 1.0          # (the second element one further out: a one-pack case is not uniform by accident)
    if D == "box":
        return D_HI + d, D_LO - d - 1.0
    if D == "box_vec":
        j = min(i + 1, len(dlo) - 1)          # (a caller that wants one element passes the last one)
        if dform == "both":
            return dhi[i] + d, dlo[j] - d - 1.0
        if dform == "lo_vec_hi_inf":
            return dlo[i] - d, dlo[j] - d - 1.0
        return dhi[i] + d, -0.6 - d - 1.0
    return {"vc": (d, -d - 3.0), "cc": (d + 3.0, d), "eitheror": (-d, -d - 3.0), "xor": (d + 3.0, d)}[D]


def class_variant(g, D):
    """the vector-bound forms of g = indbox_vec and D = box_vec, rotated over the classes so that every form runs"""
    i = G_KINDS.index(g) + D_KINDS.index(D)
    return VEC_FORMS[i % 3], VEC_FORMS[(i // 3 + i) % 3]


def class_f(g, D):
    """f of a class: DiagQuadratic, and Zero for every other class whose g has the value 0 (module docstring)"""
    return "zero" if g in ZERO_VALUED_G and (G_KINDS.index(g) + D_KINDS.index(D)) % 2 == 1 else "diag"


def class_regime(g, D):
    """the four regimes rotated over g within one D: 7 g kinds, so every regime meets every D in both types"""
    return REGIMES[(G_KINDS.index(g) + D_KINDS.index(D)) % 4]


def class_size(g, D, dtype, regime):
    """one pack / a thousand-odd / 2121-odd elements, rotated; the last pack ragged (fp64: n odd; fp32: n = 3 mod 4;
    pair sets need n even: n = 2 mod 4).  `last` never takes the one-pack size: it needs near elements too."""
    pk = pack_of(dtype)
    k = (G_KINDS.index(g) + 2 * D_KINDS.index(D)) % 3
    if k == 0 and regime == "last":
        k = 1
    if k == 0:
        return pk
    base = 1000 if k == 1 else 2120
    if D in PAIRWISE:
        return base + 2
    return base + (1 if pk == 2 else 3)


def build_oracles(m, dtype, par, f, g, D, gform, dform, layout="adjacent"):
    """(f, g, c, D) of module m (the device package or the oracle) from the vectors in par"""
    T = np.dtype(dtype).type
    device = m.__name__.split(".")[-1] != "bazinga_ref"
    num = float if device else (lambda v: T(v))          # scalar parameters: Python floats for the device
    ff = m.DiagQuadratic(par["q"], par["b"]) if f == "diag" else m.Zero()
    u, glo, ghi, dlo, dhi = (par[k] for k in ("u", "glo", "ghi", "dlo", "dhi"))
    if g == "l1":
        gg = m.NormL1(num(0.8))
    elif g == "nonneg":
        gg = m.NormL1Nonneg(num(0.8))
    elif g == "l1box":
        gg = m.NormL1Box(num(0.8), u=u)
    elif g == "l0box":
        gg = m.NormL0Box(num(0.3), u=u)
    elif g == "indbox":
        gg = m.IndBox(num(G_LO), num(G_HI))
    elif g == "indbox_vec":
        gg = {"both": lambda: m.IndBox(glo, ghi), "lo_vec_hi_inf": lambda: m.IndBox(glo, num(np.inf)),
              "lo_num_hi_vec": lambda: m.IndBox(num(G_LO), ghi)}[gform]()
    else:
        gg = m.Zero()
    if D == "box":
        DD = m.ClosedSet(m.IndBox(num(D_LO), num(D_HI)))
    elif D == "box_vec":
        DD = m.ClosedSet({"both": lambda: m.IndBox(dlo, dhi), "lo_vec_hi_inf": lambda: m.IndBox(dlo, num(np.inf)),
                          "lo_num_hi_vec": lambda: m.IndBox(num(-0.6), dhi)}[dform]())
    elif D == "free":
        DD = m.FreeSet()
    elif D == "zero":
        DD = m.ZeroSet()
    else:
        DD = m.PairwiseSet(D, layout)
    return ff, gg, m.IdentityFunction(), DD


def _parameters(rng, n, dtype):
    q = rng.uniform(0.2, 5.0, n)
    b = 4.0 * rng.standard_normal(n)
    b = np.where(np.abs(b) < 1.5, np.where(b < 0, -1.5, 1.5), b)      # |b| >= 1.5: every element's f + g is <= 0 (below)
    u = np.where(np.arange(n) % 5 == 0, 0.0, rng.uniform(0.3, 1.0, n))
    glo, ghi = -rng.uniform(0.2, 1.0, n), rng.uniform(0.2, 1.0, n)
    dlo, dhi = -rng.uniform(0.1, 1.0, n), rng.uniform(0.1, 1.0, n)
    return {k: v.astype(dtype) for k, v in (("q", q), ("b", b), ("u", u), ("glo", glo), ("ghi", ghi), ("dlo", dlo), ("dhi", dhi))}


def _plant(par, x0, i, v, q=0.25):
    """x0[i] = v, with f's and g's parameters of that element chosen so that v survives prox_g where the kind allows it and
    the element's 0.5 q v^2 - b v + g(v) is <= 0 (v between 0 and b / q; |b| = 4 beats lambda = 0.8)"""
    T = x0.dtype.type
    x0[i] = v
    par["q"][i] = T(q)
    par["b"][i] = T(-4.0 if (v < 0 or (v == 0 and np.signbit(v))) else 4.0)
    if np.isfinite(v):
        a = abs(float(v))
        par["u"][i] = max(par["u"][i], T(a + 0.5))
        par["ghi"][i] = max(par["ghi"][i], T(a + 0.5))
        par["glo"][i] = min(par["glo"][i], T(-a - 0.5))


def draw_outer_case(g, D, dtype, regime, n, f="diag", forms=None, layout="adjacent", bz=None, ref=None):
    """One case of the outer-loop table: {"dev": device oracles (None without bz), "orc": reference oracles, "x0", "y0",
    "gamma", "par"}.  f = DiagQuadratic(q, b) with q in U(0.2, 5), b = 4 N(0, 1) (|b| >= 1.5), x0 = 0.5 b / q limited to
    [-1.2, 1.2] (within sqrt(2) of every D here) with every fifth entry 0, y0 = N(0, 1).
    regime: "uni0" a few pairs of x0 at distance 3 from D (mu non-uniform); "uni1" none (mu = 0.1 everywhere), y0 != 0;
    "uni2" as uni1 with y0 = 0; "last" only the last element (pair) far."""
    dtype = np.dtype(dtype).type
    gform, dform = forms or class_variant(g, D)
    rng = np.random.default_rng(zlib.crc32(("outer-%s-%s-%s-%s-%s-%d-%s" % (f, g, D, np.dtype(dtype).name, regime, n, layout)).encode()))
    par = _parameters(rng, n, dtype)
    x0 = np.clip(0.5 * par["b"].astype(np.float64) / par["q"], -1.2, 1.2).astype(dtype)
    x0[::5] = 0
    y0 = np.zeros(n, dtype) if regime == "uni2" else rng.standard_normal(n).astype(dtype)
    if regime == "uni0":
        for i in (p for p in (0, 6, 14, n - 2 - n % 2) if p + 1 < n):
            for e, v in enumerate(pair_at_distance(D, 3.0, dform, par["dlo"], par["dhi"], i)):
                _plant(par, x0, i + e, dtype(v))
    elif regime == "last":
        if D in PAIRWISE:
            for e, v in enumerate(pair_at_distance(D, 3.0, dform, par["dlo"], par["dhi"], n - 2)):
                _plant(par, x0, n - 2 + e, dtype(v))
        else:
            # (the first value of a pair is the positive one — prox_g of the NONNEG_G kinds keeps it — except for
            # lo_vec_hi_inf, which has no upper bound to be above; no NONNEG_G class has that form)
            _plant(par, x0, n - 1, dtype(pair_at_distance(D, 3.0, dform, par["dlo"][n - 1:], par["dhi"][n - 1:], 0)[0]))
    return finish_case(g, D, dtype, f, (gform, dform), layout, par, x0, y0, bz, ref)


def finish_case(g, D, dtype, f, forms, layout, par, x0, y0, bz, ref):
    if layout == "split":      # the pairs (i, i + N) of the caller's order are the adjacent pairs drawn above
        N = x0.shape[0] // 2
        perm = np.empty(2 * N, np.int64)
        perm[0::2], perm[1::2] = np.arange(N), np.arange(N) + N
        ip = np.argsort(perm)
        par = {k: np.ascontiguousarray(v[ip]) for k, v in par.items()}
        x0, y0 = np.ascontiguousarray(x0[ip]), np.ascontiguousarray(y0[ip])
    out = {"x0": x0, "y0": y0, "gamma": GAMMA, "par": par, "dev": None, "orc": None, "key": (f, g, D, np.dtype(dtype).name)}
    for name, m in (("dev", bz), ("orc", ref)):
        if m is not None:
            out[name] = build_oracles(m, dtype, par, f, g, D, forms[0], forms[1], layout)
    return out


# ------------------------------------------------------------------ arguments where the arithmetic branches
def special_outer_case(g, D, dtype, n, mode, bz=None, ref=None, f="diag"):
    """x0 and y0 with the values where the outer loop's element arithmetic branches.
    y0: +-1e20 (the safeguard's bounds) with their neighbours on both sides, +-3e20, +-0, a subnormal; x0: the bounds of D
    (the scalar ones and each element's own), distances from D around sqrt(2) (0.5 d^2 around 1: where mu leaves 0.1), a
    distance at which mu meets its 1e8 clamp, and for the pair sets every ordered pair of the tie values of
    test_pairwise_sets_every_special_pair_bit_exact.
    mode "finite": those alone; "nan_y": y0 also holds +-inf and NaN; "nan_x": x0 also holds +-inf and NaN (and the pairs
    with them)."""
    dtype = np.dtype(dtype).type
    T = dtype
    gform, dform = class_variant(g, D)
    rng = np.random.default_rng(zlib.crc32(("special-%s-%s-%s-%d" % (g, D, np.dtype(dtype).name, n)).encode()))
    par = _parameters(rng, n, dtype)
    x0 = np.clip(0.5 * par["b"].astype(np.float64) / par["q"], -1.2, 1.2).astype(dtype)
    x0[::5] = 0
    y0 = rng.standard_normal(n).astype(dtype)
    inf, big = T(np.inf), T(1e20)
    ys = [big, -big, np.nextafter(big, inf), np.nextafter(big, -inf), np.nextafter(-big, inf), np.nextafter(-big, -inf),
          T(3e20), T(-3e20), T(0.0), T(-0.0), np.finfo(dtype).tiny / T(4), T(1e-30)]
    if mode == "nan_y":
        ys += [inf, -inf, T(np.nan)]
    for k, v in enumerate(ys):
        for rep in range(3):          # (three elements per value, spread: every fifth x0 is 0)
            y0[(7 * k + 3 + rep * 7 * len(ys)) % n] = v
    y0[n - 1] = ys[(n + len(g)) % len(ys)]          # ... and one in the ragged last pack
    # x0, element values
    r2 = T(np.sqrt(T(2)))
    dists = [np.nextafter(np.nextafter(r2, -inf), -inf), np.nextafter(r2, -inf), r2, np.nextafter(r2, inf),
             np.nextafter(np.nextafter(r2, inf), inf), T(0.0), T(1e-30), T(4.5e4), T(1e5)]
    pos = 40
    for d in dists:
        for rep in range(2):
            i = pos + 2 * (pos % 3)          # an even index
            for e, v in enumerate(pair_at_distance(D, float(d), dform, par["dlo"], par["dhi"], i)):
                v = T(v)
                _plant(par, x0, i + e, v, q=0.25 if abs(v) < 30 else 1e-12)
            pos += 10
    xs = [T(D_LO), T(D_HI), T(-0.6), T(0.0), T(-0.0), np.finfo(dtype).tiny / T(4)]
    if mode == "nan_x":
        xs += [inf, -inf, T(np.nan)]
    for k, v in enumerate(xs):
        for rep in range(3):
            _plant(par, x0, 301 + 4 * k + 50 * rep, v)
    for i in range(500, 540):          # each element's own bounds of D = box_vec
        _plant(par, x0, i, par["dhi"][i] if i % 2 else par["dlo"][i])
    if D in PAIRWISE:
        sp = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1e-30, -1e-30, float(np.finfo(dtype).tiny) / 4,
              -float(np.finfo(dtype).tiny) / 4]
        if mode == "nan_x":
            sp += [np.inf, -np.inf, np.nan]
        i = 600
        for a in sp:
            for b_ in sp:
                _plant(par, x0, i, T(a))
                _plant(par, x0, i + 1, T(b_))
                i += 2
        assert i <= n
    return finish_case(g, D, dtype, f, (gform, dform), "adjacent", par, x0, y0, bz, ref)


SPECIAL_N = {("float64", False): 1201, ("float32", False): 1203, ("float64", True): 1202, ("float32", True): 1202}


def special_classes():
    """every D in both types, g = zero (the planted values reach the outer arithmetic unchanged) and one more g, rotated"""
    out = []
    for ti, dt in enumerate(TYPES):
        for di, D in enumerate(D_KINDS):
            out.append(("zero", D, dt))
            out.append((G_KINDS[1 + (2 * di + ti) % 6], D, dt))
    return out


# ------------------------------------------------------------------ the oracle's outer loop, state by state
class _RecordingSet:
    """D with the last projection kept: the oracle's s at an outer iteration (its trace does not carry it)"""

    def __init__(self, D):
        self.D, self.last = D, None

    def proj(self, z, x):
        self.D.proj(z, x)
        self.last = np.array(z, copy=True)


def sub_factory(m, gamma=GAMMA):
    return lambda **kw: m.PANOCplus(maxit=1, gamma=gamma, adaptive=False, **kw)


def oracle_states(ref, case, K=K_OUTER, solver="alps", **kw):
    """What ref.alps(..., maxit=k) returns for k = 1 .. K, from ONE run with maxit = K: entries (x, y, tot_it, tot_inner_it,
    status, inner_tol, norm_res_prim, s, mu) per k, then per iteration the penalties and multipliers the subproblem ran
    with, and the theta decisions (iteration, taken, norm_res_prim, theta * old).
    A run that ends at K' < K ended for good: maxit = k > K' returns the same state."""
    f, g, c, D = case["orc"]
    rec = _RecordingSet(D)
    rows, entering, decisions = [], [], []
    theta = kw.get("theta_penalty", 0.8)
    T = case["x0"].dtype.type
    tol_prim = kw.get("tol", T(1e-6))
    y_in = [np.maximum(-1e20, np.minimum(case["y0"], 1e20)).astype(case["y0"].dtype)]

    def trace(tot_it, x, y, mu, sub_it, inner_tol, nrp, objx):
        rows.append((x.copy(), y.copy(), tot_it, tot_it * 1, inner_tol, nrp, rec.last.copy(), mu.copy()))
        entering.append((mu.copy(), y_in[-1]))
        y_in.append(y.copy())
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if solver == "alps":
            o = ref.alps(f, g, c, rec, case["x0"], case["y0"].copy(), maxit=K, subsolver=sub_factory(ref, case["gamma"]),
                         outer_trace=trace, **kw)
        else:
            raise ValueError(solver)
    states = []
    for k in range(1, K + 1):
        if k >= o[2]:
            states.append((o[0], o[1], o[2], o[3], o[5], o[6], o[7], o[8], o[9]))
        else:
            x, y, it, inner, itol, nrp, s, mu = rows[k - 1]
            states.append((x, y, it, inner, "max_iter", itol, nrp, s, mu))
    for k in range(2, o[2]):          # (the theta test runs at iterations 2 .. tot_it - 1: not at the first, not at the last)
        nrp, old = rows[k - 1][5], rows[k - 2][5]
        # (in double, as Julia's theta_penalty::Float64 * norm_res_prim_old promotes)
        decisions.append((k, float(nrp) > max(theta * float(old), float(tol_prim)), float(nrp), theta * float(old)))
    return states, entering, decisions


def uni_of(mu, y):
    """P.uni as the probe of k_muy should report it: 1 uniform penalties, 2 and zero scaled multipliers"""
    if not np.all(mu == mu[0]):
        return 0
    with np.errstate(all="ignore"):
        return 2 if np.all(mu * y == 0) else 1


def table_cases():
    """(g, D, type, layout) of test_alps_outer_loop_bit_for_bit: every (g, D, type) once, and one split-layout pair set"""
    out = [(g, D, dt, "adjacent") for dt in TYPES for D in D_KINDS for g in G_KINDS]
    out += [("l1", "cc", dt, "split") for dt in TYPES]
    return out


# theta_penalty of a case: 0.8 (the default) and, for every third class, 3.0 — a residual that grows by less than that
# leaves the penalties alone, so the not-taken branch of the theta test runs beside a constrained D too
def class_theta(g, D):
    return 3.0 if (G_KINDS.index(g) + D_KINDS.index(D)) % 3 == 2 else 0.8


def table_case(g, D, dt, layout, bz=None, ref=None):
    regime = class_regime(g, D)
    n = class_size(g, D, dt, regime)
    if layout == "split":
        regime, n = "uni0", 1002
    return draw_outer_case(g, D, dt, regime, n, f=class_f(g, D), layout=layout, bz=bz, ref=ref), regime, n


def als_cases():
    return [(g, D, dt) for dt in TYPES for D in SLACK_D_KINDS for g in G_KINDS]


def als_case(g, D, dt, bz=None, ref=None):
    """the slack form needs nx to be a multiple of the pack: one pack, 1000 or 2120 elements (nx / pack is no multiple of
    the 256-thread block: the grid is ragged instead of the pack)"""
    regime = class_regime(g, D)
    k = (G_KINDS.index(g) + 2 * D_KINDS.index(D)) % 3
    if k == 0 and regime == "last":
        k = 1
    n = (pack_of(dt), 1000, 2120)[k]
    return draw_outer_case(g, D, dt, regime, n, f=class_f(g, D), bz=bz, ref=ref), regime, n


def theta_tie_case(dt, bz=None, ref=None):
    """norm_res_prim == theta_penalty * norm_res_prim_old EXACTLY at every decision, with theta_penalty = 1: g = IndBox
    pins one element at its upper bound G_HI (b = 400 there: the gradient stays negative through every halving) while D's
    box ends at D_HI, so that element's residual G_HI - D_HI is the largest one, iteration after iteration.  The test
    `norm_res_prim > max(theta * old, tol_prim)` is strict: the penalties are never scaled."""
    n = 1001 if dt == "float64" else 1003
    case = draw_outer_case("indbox", "box", dt, "uni1", n, bz=None, ref=None)
    par, x0 = case["par"], case["x0"]
    _plant(par, x0, 7, x0.dtype.type(G_HI))
    par["b"][7] = 400.0
    return finish_case("indbox", "box", x0.dtype.type, "diag", class_variant("indbox", "box"), "adjacent", par, x0, case["y0"],
                       bz, ref)


# ------------------------------------------------------------------ the outer loop beside a matrix (sums have an order)
MATRIX_KINDS = ("dense_alps", "sparse_alps", "dense_als", "spls_identity")
MATRIX_SHAPES = ((20, 100), (41, 121))
MATRIX_D = ("zero", "box", "box_vec")
K_MATRIX = 4
CUT_ROWS = (257, 1031)          # at density 0.9 its rows are longer than a segment (tests/test_gpu_sparse.py)


def matrix_cases():
    out = [(k, s, D, dt) for dt in TYPES for k in MATRIX_KINDS for s in MATRIX_SHAPES for D in MATRIX_D]
    return out + [("sparse_alps", CUT_ROWS, "box", "float64"), ("sparse_alps", CUT_ROWS, "zero", "float32")]


class CsrOracle:
    """eval!(cx, c, x) = A x - b, jtprod!(jtv, c, x, v) = A'v over CSR arrays (the duck-type of tests/test_gpu_sparse.py)"""

    def __init__(self, indptr, indices, data, b, n):
        self.indices, self.data, self.b, self.n = np.asarray(indices), np.asarray(data), np.asarray(b), n
        self.ny = self.b.shape[0]
        self.rows = np.repeat(np.arange(self.ny), np.diff(indptr))

    def eval(self, cx, x):
        cx[...] = np.bincount(self.rows, weights=self.data * x[self.indices], minlength=self.ny) - self.b

    def jtprod(self, jtv, x, v):
        jtv[...] = np.bincount(self.indices, weights=self.data * v[self.rows], minlength=self.n)


def _csr(A):
    indptr = np.concatenate(([0], np.cumsum(np.count_nonzero(A, axis=1)))).astype(np.int64)
    rows, cols = np.nonzero(A)
    return indptr, cols.astype(np.int32), A[rows, cols]


def matrix_case(kind, shape, D, dt, bz=None, ref=None):
    """{"dev", "orc", "x0", "y0", "gamma", "solver"}: f = DiagQuadratic, g = NormL1(0.8) beside c(x) = A x - b (dense, or
    CSR) under alps or als; or f = SparseLeastSquares beside c = Identity from a start whose objective is above 1 — there
    the penalty denominator max(1, objx) is a reduced value."""
    dtype = np.dtype(dt).type
    m, n = shape
    if kind == "dense_als":
        n = n // 4 * 4          # (the slack form needs nx to be a multiple of the pack: 41 x 120 there, the rows stay odd)
    rng = np.random.default_rng(zlib.crc32(("matrix-%s-%dx%d-%s-%s" % (kind, m, n, D, dt)).encode()))
    if kind.startswith("dense"):
        A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(dtype)
    else:
        p = 0.9 if shape == CUT_ROWS else 0.3
        A = ((rng.standard_normal((m, n)) / np.sqrt(p * n)) * (rng.random((m, n)) < p)).astype(dtype)
    ny = n if kind == "spls_identity" else m
    par = _parameters(rng, n, dtype)
    dlo, dhi = (-rng.uniform(0.1, 1.0, ny)).astype(dtype), rng.uniform(0.1, 1.0, ny).astype(dtype)
    y0 = rng.standard_normal(ny).astype(dtype)
    if kind == "spls_identity":
        x0 = (0.3 * rng.standard_normal(n)).astype(dtype)
        x0[3::17] = 3.0
        bf = rng.standard_normal(m).astype(dtype)
    else:
        x0 = np.clip(0.5 * par["b"].astype(np.float64) / par["q"], -1.2, 1.2).astype(dtype)
        x0[::5] = 0
        bc = (0.3 * rng.standard_normal(m)).astype(dtype)
    out = {"x0": x0, "y0": y0, "gamma": 0.001 if kind == "spls_identity" else GAMMA, "solver": "als" if kind == "dense_als" else "alps",
           "dev": None, "orc": None}
    for name, mod in (("dev", bz), ("orc", ref)):
        if mod is None:
            continue
        device = name == "dev"
        num = float if device else (lambda v: dtype(v))
        DD = {"zero": lambda: mod.ZeroSet(), "box": lambda: mod.ClosedSet(mod.IndBox(num(D_LO), num(D_HI))),
              "box_vec": lambda: mod.ClosedSet(mod.IndBox(dlo, dhi))}[D]()
        if kind == "spls_identity":
            ff = mod.SparseLeastSquares(*_csr(A), bf, n) if device else mod.LeastSquares(A, bf)
            cc = mod.IdentityFunction()
        else:
            ff = mod.DiagQuadratic(par["q"], par["b"])
            if kind == "sparse_alps":
                cc = mod.SparseAffine(*_csr(A), bc, n) if device else CsrOracle(*_csr(A), bc, n)
            else:
                cc = mod.DenseAffine(A, bc)
        out[name] = (ff, mod.NormL1(num(0.8)), cc, DD)
    return out


def matrix_oracle_runs(ref, case, reducer=None):
    """ref.alps / ref.als with maxit = 1 .. K_MATRIX; reducer: the oracle's sums carried by it (the twin of the envelope)"""
    runs = []
    solve = ref.als if case["solver"] == "als" else ref.alps
    ref.set_reducer(reducer)
    try:
        for k in range(1, K_MATRIX + 1):
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                runs.append(solve(*case["orc"], case["x0"], case["y0"].copy(), maxit=k, subsolver=sub_factory(ref, case["gamma"])))
    finally:
        ref.set_reducer(None)
    return runs


# ------------------------------------------------------------------ the preconditions
def _objective_at_start(ref, case):
    f, g = case["orc"][0], case["orc"][1]
    x = np.empty_like(case["x0"])
    with np.errstate(all="ignore"):
        gz = g.prox(x, case["x0"], np.finfo(x.dtype).eps)
        return float(f(x) + gz), x


@pytest.fixture(scope="module")
def table(ref):
    out = {}
    for c in table_cases():
        case, regime, n = table_case(*c, ref=ref)
        out[c] = (case, regime, n) + oracle_states(ref, case, theta_penalty=class_theta(c[0], c[1]))
    return out


def test_every_class_regime_and_size_is_in_the_table():
    cases = table_cases()
    assert {(g, D, dt) for g, D, dt, _ in cases} == {(g, D, dt) for g in G_KINDS for D in D_KINDS for dt in TYPES}
    for D in D_KINDS:
        assert {class_regime(g, D) for g in G_KINDS} == set(REGIMES), D
        for dt in TYPES:
            sizes = {class_size(g, D, dt, class_regime(g, D)) for g in G_KINDS}
            assert len(sizes) == 3 and min(sizes) == pack_of(dt), (D, dt, sizes)
            for n in sizes:
                assert n == pack_of(dt) or (n % 2 == 0 and n % 4 == 2 if D in PAIRWISE else n % pack_of(dt) == pack_of(dt) - 1)
    assert {class_f(g, D) for g in G_KINDS for D in D_KINDS} == {"diag", "zero"}
    assert {class_variant("zero", "box_vec")[1], class_variant("l1", "box_vec")[1], class_variant("nonneg", "box_vec")[1]} \
        == set(VEC_FORMS)


def test_start_objective_keeps_the_penalty_denominator_at_one(ref, table):
    for c, (case, regime, n, states, entering, decisions) in table.items():
        objx, _ = _objective_at_start(ref, case)
        assert objx <= 1.0, (c, regime, n, objx)


def test_states_stay_finite_and_small(table):
    for c, (case, regime, n, states, entering, decisions) in table.items():
        for k, st in enumerate(states):
            for v in (st[0], st[1], st[7], st[8]):
                assert np.all(np.isfinite(v)) and np.max(np.abs(v)) < 1e6, (c, regime, n, k + 1)
            assert np.isfinite(st[6]) and st[6] < 1e6


def test_regimes_give_the_penalties_they_promise(table):
    """uni0 / last: non-uniform penalties wherever an argument can be far from D at all; last: the last element (pair) is
    the only one that differs; uni1: mu = 0.1 everywhere and mu * y != 0; uni2: zero multipliers at the first iteration
    only."""
    seen = set()
    for c, (case, regime, n, states, entering, decisions) in table.items():
        g, D, dt, layout = c
        mu1 = entering[0][0]
        u = [uni_of(m, y) for m, y in entering]
        seen.add((regime, u[0]))
        if regime in ("uni0", "last") and not cannot_be_far(g, D):
            assert u[0] == 0 and mu1.max() > 0.25, (c, regime, n)
            if regime == "last":
                far = np.flatnonzero(mu1 != mu1.dtype.type(0.1))
                assert far.size and far.min() >= n - 2 + (D not in PAIRWISE), (c, far)
        elif regime == "uni2":
            assert u[0] == 2 and np.all(mu1 == mu1.dtype.type(0.1)), (c, regime, n)
            # (D = Free, or a one-pack case that starts inside D: y = (cx + mu y - s) / mu stays 0 throughout)
            assert all(v == 2 for v in u[1:]) if D == "free" else all(v in (1, 2) for v in u[1:]), (c, u)
            assert cannot_be_far(g, D) or n == pack_of(dt) or (len(u) >= 2 and u[1] == 1), (c, u)
        else:
            assert u[0] == 1 and np.all(mu1 == mu1.dtype.type(0.1)), (c, regime, n, u)
    assert {(r, v) for r, v in seen if r in ("uni0", "last")} >= {("uni0", 0), ("last", 0)}


def test_both_outcomes_of_the_theta_test_occur_for_every_constrained_set(table):
    """per (D, type): the penalty update is taken in some case and skipped in another (D = Free has residual 0: it never
    scales, and stops first_order instead)"""
    for dt in TYPES:
        for D in D_KINDS:
            taken = set()
            for c, (case, regime, n, states, entering, decisions) in table.items():
                if c[1] == D and c[2] == dt:
                    taken |= {t for _, t, _, _ in decisions}
            if D == "free":
                assert taken == {False}, (D, dt, taken)
                assert any(v[3][-1][4] == "first_order" for c, v in table.items() if c[1] == D and c[2] == dt)
            else:
                assert taken == {True, False}, (D, dt, taken)


def test_one_run_gives_the_states_of_every_maxit(ref, table):
    """oracle_states against ref.alps(maxit = k) itself, on three classes (one of them stops early)"""
    for c in (("l1", "box", "float64", "adjacent"), ("zero", "free", "float32", "adjacent"), ("indbox", "xor", "float32", "adjacent")):
        case, regime, n, states, _, _ = table[c]
        for k in range(1, K_OUTER + 1):
            with np.errstate(all="ignore"):
                o = ref.alps(*case["orc"], case["x0"], case["y0"].copy(), maxit=k, subsolver=sub_factory(ref),
                             theta_penalty=class_theta(c[0], c[1]))
            got = (o[0], o[1], o[2], o[3], o[5], o[6], o[7], o[8], o[9])
            for a, b in zip(got, states[k - 1]):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, (c, k)


@pytest.mark.parametrize("mode", ["finite", "nan_y", "nan_x"])
def test_special_arguments_reach_their_branches(ref, mode):
    """the planted arguments of test_outer_arguments_where_the_arithmetic_branches: the finite run keeps the denominator at 1
    and reaches both sides of every clamp; a NaN multiplier ends the oracle's run as :exception after one iteration, a NaN
    in x0 before the first.  (With maxit = 1 the status is :max_iter either way — `tired` is asked before `broken` — so
    the status is read from maxit = 2: the oracle still stops after the first iteration.)"""
    for g, D, dt in special_classes():
        n = SPECIAL_N[(dt, D in PAIRWISE)]
        case = special_outer_case(g, D, dt, n, mode, ref=ref)
        objx, x = _objective_at_start(ref, case)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            o = ref.alps(*case["orc"], case["x0"], case["y0"].copy(), maxit=1 if mode == "finite" else 2,
                         subsolver=sub_factory(ref))
        T = np.dtype(dt).type
        if mode == "finite":
            assert objx <= 1.0, (g, D, dt, objx)
            assert o[2] == 1 and o[5] == "max_iter"
            assert np.all(np.isfinite(o[1])) and np.all(np.isfinite(o[9]))
            if g == "zero" and D != "free":
                assert o[9].max() == T(1e8) and o[9].min() == T(0.1) and np.unique(o[9]).size >= 4, (D, dt, np.unique(o[9]))
        elif mode == "nan_y":
            assert objx <= 1.0 and np.isnan(o[1]).sum() >= 3, (g, D, dt, objx)
            if g in ("zero", "l1"):          # (NormL1Nonneg and the box kinds map a NaN argument to a number)
                assert o[2] == 1 and o[5] == "exception" and np.isnan(o[0]).sum() >= 3, (g, D, dt, o[5])
        else:
            # (a g that maps NaN to a number — NormL1Nonneg's where(x >= t, x - t, 0) — leaves an infinite objective)
            if g in ("zero", "l1"):
                assert o[2] == 0 and o[5] == "exception" and o[7] is None, (g, D, dt, o[5])
            if g == "zero" and D != "free":
                assert np.isnan(o[9]).any()


def test_als_cases_keep_the_denominator_at_one_and_stay_finite(ref):
    """the slack-form table: the same preconditions on ref.als, and both outcomes of the theta test per (D, type)"""
    for dt in TYPES:
        for D in SLACK_D_KINDS:
            taken = set()
            for g in G_KINDS:
                case, regime, n = als_case(g, D, dt, ref=ref)
                assert _objective_at_start(ref, case)[0] <= 1.0, (g, D, dt)
                T = np.dtype(dt).type
                theta, nrp = class_theta(g, D), []
                for k in range(1, K_OUTER + 1):
                    with np.errstate(all="ignore"), warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        o = ref.als(*case["orc"], case["x0"], case["y0"].copy(), maxit=k, subsolver=sub_factory(ref),
                                    theta_penalty=theta)
                    for v in (o[0], o[1], o[8], o[9]):
                        assert np.all(np.isfinite(v)) and np.max(np.abs(v)) < 1e6, (g, D, dt, k)
                    if o[2] == k:
                        nrp.append(float(o[7]))
                taken |= {nrp[k] > max(theta * nrp[k - 1], float(T(1e-6))) for k in range(1, len(nrp) - 1)}
            assert taken == {True, False}, (D, dt, taken)          # (D = Free too: s is a variable here, x - s is not 0)


def test_matrix_cases_are_decided_with_a_margin(ref):
    """beside a matrix a sum's order moves the last bits: every theta decision of these cases has
    |norm_res_prim - theta * old| >= 1e-6 * norm_res_prim, so no rounding flips it; the values stay finite and small; the
    SparseLeastSquares cases start from an objective above 1 (their penalty denominator is a sum), the others below"""
    taken = set()
    for c in matrix_cases():
        case = matrix_case(*c, ref=ref)
        runs = matrix_oracle_runs(ref, case)
        objx = _objective_at_start(ref, case)[0]
        assert objx > 2.0 if c[0] == "spls_identity" else objx <= 1.0, (c, objx)
        tol = float(np.dtype(c[3]).type(1e-6))
        for k, o in enumerate(runs):
            assert o[2] == k + 1 and o[5] == "max_iter", (c, k, o[2], o[5])
            for v in (o[0], o[1], o[8], o[9]):
                assert np.all(np.isfinite(v)) and np.max(np.abs(v)) < 1e6, (c, k)
        nrp = [float(o[7]) for o in runs]
        for k in range(1, len(nrp) - 1):
            assert abs(nrp[k] - 0.8 * nrp[k - 1]) >= 1e-6 * nrp[k] and nrp[k] > 10 * tol, (c, k, nrp)
            taken.add((c[0], nrp[k] > 0.8 * nrp[k - 1]))
    assert {k for k, _ in taken} == set(MATRIX_KINDS) and {t for _, t in taken} == {True, False}, taken


@pytest.mark.parametrize("dt", TYPES)
def test_theta_tie_case_ties_at_every_decision(ref, dt):
    case = theta_tie_case(dt, ref=ref)
    T = np.dtype(dt).type
    assert _objective_at_start(ref, case)[0] <= 1.0
    states, _, decisions = oracle_states(ref, case, theta_penalty=1.0)
    assert len(decisions) == K_OUTER - 2
    for k, taken, nrp, bound in decisions:
        assert nrp == bound == float(T(G_HI) - T(D_HI)) and not taken, (k, taken, nrp, bound)
    assert np.array_equal(states[-1][8], states[0][8])          # mu never scaled
