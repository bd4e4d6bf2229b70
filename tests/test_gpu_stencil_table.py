"""The 5-point-stencil path (f = Stencil5ptQuadratic, c = Identity: k_algrad_stencil, k_stencil_fb, k_stencil_update,
k_stencil_update_c, k_compact_xd) against the oracle over every g kind and D class it takes at run time, in fp64 and
fp32, with the penalties streamed (P.uni = 0) and carried as numbers (P.uni = 1 / 2).  A class is (g, D):
  g in {zero, l1, nonneg, l1box (vector u with zeros in it), l0box, indbox, indbox_vec}, D in {zero, free, box, box_vec};
the three vector-bound forms (both sides vectors, a vector below +inf, a number below a vector) rotate over the classes.
b is standard normal, lambda = 0.1, the scalar boxes are +-0.5; the near start is x0 = 0.3 N(0, 1), y = N(0, 1), the far
start x0 = 3 N(0, 1), y = 5 N(0, 1).  Every generator is seeded from the class name.
  (a) one AL gradient, bit for bit, on grids with one and two packs per row, one grid row, rows that are no power of two,
      and on one workgroup (every thread owns several chunks); unit impulses, NaN and +inf at corners, edges and an
      interior point of a 5 x 8 grid; creation refuses ny % pack != 0;
  (b) 30 states against the oracle on 24 x 32, per-element penalties and one uniform regime per class, in the library's
      default form (k_stencil_update_c) and, for every second class, with the two-loop kernels (k_stencil_update);
  (c) the fast passes (REGX = 1 and 0, penalties carried and streamed) against the generic kernel chain, bit for bit after
      every one of 40 steps on 48 x 64, in both forms of the L-BFGS operator, through tau backtracks and gamma halvings;
  (d) the non-temporal instantiations against the default-policy ones, bit for bit, at sizes past their thresholds;
  (e) whole solves, resident and through the host outer loop, against ref.alps.

What the conditions of (b) and (c) rest on, from the oracle alone (CPU, this file's generator: `python -m
tests.test_gpu_stencil_table` prints it; 28 classes x 3 regimes x 2 types, and the far starts, in 10 s):
  (b) 24 x 32, near start, 30 states, the oracle against its extended-precision twin (LongDoubleReducer):
      fp64 — 82 of the 84 runs have all 30 states tight (iter_tol(sens) == 1e-10); the other two are (zero, box) with 27
      and (zero, box_vec) with 28, both in uni0 (envelopes 1.0e-12 and 1.5e-12 after 30 states).  Asked for: 25.
      fp32 — the fewest tight states (max(2e-5, 100 sens) <= 1e-3) are 12: (l1, box) and (indbox, box_vec), both in uni0.
      Asked for: 8.
      l0box (a discontinuous prox) — 30 tight states in every regime and both types (envelope <= 4.7e-14 in fp64,
      8.1e-6 in fp32), so the twin keeps the condition for it and the class runs in (b) like the others; (c) covers it
      besides, its base form's prox tied to the oracle by test_prox_bit_exact.
      (The bound depends on the draw: of sixteen seed prefixes tried, the fewest tight states ranged from 11 to 30 in fp64
      and from 6 to 14 in fp32, nearly always in uni0 with a box D — penalties down to 0.01 beside active bounds.  SEED is
      one that keeps both conditions with room to spare; the bounds were set before the draw, not fitted to it.)
  (c) 48 x 64, far start, per-element penalties, 40 steps (two-loop oracle): tau backtracks in 11 of 28 classes in fp64
      and in 10 in fp32, gamma halvings after the start in 15 and in 11.  The device's own counters over the table's 56
      runs per type (the uniform near-start runs included): 18 with a tau backtrack and 27 with a gamma halving in fp64,
      11 and 14 in fp32.  Asked for: 4 and 8.
On an MI355X the file's 450 tests take 23 s.
"""
import zlib

import numpy as np
import pytest

from tests.test_gpu_families import SCALARS
from tests.test_gpu_parity import RTOL_ITER, LongDoubleReducer, _err, iter_tol, run_traces

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

G_KINDS = ("zero", "l1", "nonneg", "l1box", "l0box", "indbox", "indbox_vec")
D_KINDS = ("zero", "free", "box", "box_vec")
CLASSES = [(g, D) for g in G_KINDS for D in D_KINDS]
assert len(CLASSES) == 28
VEC_FORMS = ("both", "lo_vec_hi_inf", "lo_num_hi_vec")
TYPES = ("float64", "float32")
REGIMES = ("uni0", "uni1", "uni2")
# the prefix of every generator's seed (see the docstring, (b))
SEED = "st-"
# every knob that changes which stencil kernel, instantiation or grid runs
KNOBS = ("BZ_GRID", "BZ_UNI", "BZ_STENCIL_REGX", "BZ_XDNT", "BZ_SUC_GRID", "BZ_NT", "BZ_XR", "BZ_GFC", "BZ_TRIALFUSE")


def cid(cls):
    return "-".join(cls)


def variant(cls):
    """the vector-bound form of a class's IndBox g / Box D (rotated over the classes, so every form is run with each)"""
    i = G_KINDS.index(cls[0]) + D_KINDS.index(cls[1])
    return VEC_FORMS[i % 3], VEC_FORMS[i % 3]


def uniform_regime(cls):
    """the uniform regime of a class in (b) and (c): uni1 and uni2 alternate over g and over D"""
    return "uni1" if (G_KINDS.index(cls[0]) + D_KINDS.index(cls[1])) % 2 == 0 else "uni2"


def also_two_loop(cls):
    """every second class, two of the four D per g, rotated with g (so that both uniform regimes are among them)"""
    gi, di = G_KINDS.index(cls[0]), D_KINDS.index(cls[1])
    return di in (gi % 4, (gi + 1) % 4)


def make_case(bz, ref, nx, ny, cls, dtype, regime, far=False):
    """(device oracles, reference oracles, mu, y, x0) of class `cls` on an nx-by-ny grid in type `dtype`.
    regime: "uni0" per-element mu in 10^U(-2, 0) and y != 0; "uni1" uniform mu = 0.1, y != 0; "uni2" uniform mu, y = 0."""
    g, D = cls
    n = nx * ny
    T = np.dtype(dtype).type
    gform, dform = variant(cls)
    r = np.random.default_rng(zlib.crc32((SEED + cid(cls)).encode()))
    b = r.standard_normal(n).astype(dtype)
    u = np.where(np.arange(n) % 5 == 0, 0.0, r.uniform(0.3, 1.0, n)).astype(dtype)
    glo, ghi = (-r.uniform(0.2, 1.0, n)).astype(dtype), r.uniform(0.2, 1.0, n).astype(dtype)
    dlo, dhi = (-r.uniform(0.1, 1.0, n)).astype(dtype), r.uniform(0.1, 1.0, n).astype(dtype)
    out = []
    for m in (bz, ref):
        # (scalar parameters: numbers of the type for the oracle, Python floats for the device)
        num = (lambda v: T(v)) if m is ref else float
        box = {"both": lambda lo, hi, s: m.IndBox(lo, hi), "lo_vec_hi_inf": lambda lo, hi, s: m.IndBox(lo, num(np.inf)),
               "lo_num_hi_vec": lambda lo, hi, s: m.IndBox(num(s), hi)}
        gg = {"zero": lambda: m.Zero(), "l1": lambda: m.NormL1(num(0.1)), "nonneg": lambda: m.NormL1Nonneg(num(0.1)),
              "l1box": lambda: m.NormL1Box(num(0.1), u=u), "l0box": lambda: m.NormL0Box(num(0.1), u=u),
              "indbox": lambda: m.IndBox(num(-0.5), num(0.5)), "indbox_vec": lambda: box[gform](glo, ghi, -0.4)}[g]()
        DD = {"zero": lambda: m.ZeroSet(), "free": lambda: m.FreeSet(),
              "box": lambda: m.ClosedSet(m.IndBox(num(-0.5), num(0.5))),
              "box_vec": lambda: m.ClosedSet(box[dform](dlo, dhi, -0.6))}[D]()
        out.append((m.Stencil5ptQuadratic(nx, ny, b), gg, m.IdentityFunction(), DD))
    rng = np.random.default_rng(zlib.crc32(("%s%s-%s-%s-%d" % (SEED, cid(cls), np.dtype(dtype).name, regime, far)).encode()))
    mu = (10.0 ** rng.uniform(-2, 0, n)).astype(dtype) if regime == "uni0" else np.full(n, 0.1, dtype)
    yn = ((5.0 if far else 1.0) * rng.standard_normal(n)).astype(dtype)
    y = np.zeros(n, dtype) if regime == "uni2" else yn
    x0 = ((3.0 if far else 0.3) * rng.standard_normal(n)).astype(dtype)
    return out[0], out[1], mu, y, x0


def clear_knobs(monkeypatch, **env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


# ------------------------------------------------------------------ (a) one AL gradient
SHAPES = {"float64": [(1, 2), (2, 2), (1, 4), (5, 2), (3, 6), (17, 34), (64, 130)],
          "float32": [(1, 4), (2, 4), (1, 8), (5, 4), (3, 12), (17, 36), (64, 132)]}
ONE_WORKGROUP = (40, 48)      # under BZ_GRID=1: a chunk's north / south rows belong to other threads


def _oracle_gradient(ref, orc, mu, y, x):
    with np.errstate(all="ignore"):
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x)
        g_ref = np.empty_like(x)
        lx = al.gradient(g_ref, x)
    return g_ref, float(lx), float(al.fx)


def _value_tol(dt):
    # (the numbers of test_stencil_al_gradient_bit_exact and of the sparse tests)
    return 1e-12 if dt == "float64" else 2e-5


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("cls", CLASSES, ids=cid)
def test_stencil_al_gradient_bit_exact_over_the_table(bz, ref, monkeypatch, cls, dt, regime):
    """gradient!(dlx, al, x) element-wise bit-exact, L(x) and f(x) to 1e-12 / 2e-5 of max(1, |L|)."""
    dtype = np.dtype(dt).type
    for shape, grid in [(s, None) for s in SHAPES[dt]] + [(ONE_WORKGROUP, "1")]:
        clear_knobs(monkeypatch, **({"BZ_GRID": grid} if grid else {}))
        nx, ny = shape
        n = nx * ny
        dev, orc, mu, y, x = make_case(bz, ref, nx, ny, cls, dtype, regime)
        prob = bz.Problem(*dev, n, n, dtype)
        try:
            prob.set_multipliers(mu, y)
            g_dev, vals = prob.eval_al_gradient(x)
        finally:
            prob.close()
        g_ref, lx, fx = _oracle_gradient(ref, orc, mu, y, x)
        assert np.array_equal(g_dev, g_ref), (shape, int(np.sum(g_dev != g_ref)))
        tol = _value_tol(dt) * max(1.0, abs(lx))
        assert abs(vals[0] - lx) <= tol and abs(vals[1] - fx) <= tol, (shape, vals[0], lx, vals[1], fx)


# corners, one point on each edge and an interior point of 5 x 8 (fp32: column 3 is the last element of the row's first
# pack, column 4 the first of its second: the impulse is the east neighbour of one pack and the west neighbour of the other)
IMPULSE_GRID = (5, 8)
IMPULSE_POINTS = [(0, 0), (0, 7), (4, 0), (4, 7), (0, 4), (4, 3), (2, 0), (2, 7), (2, 3)]


def _pattern(v):
    v = np.asarray(v, dtype=np.float64)
    return np.isnan(v), np.isposinf(v), np.isneginf(v)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("D", D_KINDS)
def test_stencil_al_gradient_of_impulses(bz, ref, monkeypatch, D, dt, regime):
    """x = e_k: bit for bit.  x = NaN e_k, x = +inf e_k: the oracle's NaN / inf pattern in the gradient, in L(x) and in
    f(x), every finite entry of the gradient bit-equal."""
    clear_knobs(monkeypatch)
    dtype = np.dtype(dt).type
    nx, ny = IMPULSE_GRID
    n = nx * ny
    dev, orc, mu, y, _ = make_case(bz, ref, nx, ny, ("zero", D), dtype, regime)
    prob = bz.Problem(*dev, n, n, dtype)
    try:
        prob.set_multipliers(mu, y)
        for i, j in IMPULSE_POINTS:
            for v in (1.0, np.nan, np.inf):
                x = np.zeros(n, dtype)
                x[i * ny + j] = v
                g_dev, vals = prob.eval_al_gradient(x)
                g_ref, lx, fx = _oracle_gradient(ref, orc, mu, y, x)
                tag = (i, j, v)
                if v == 1.0:
                    assert np.array_equal(g_dev, g_ref), tag
                    tol = _value_tol(dt) * max(1.0, abs(lx))
                    assert abs(vals[0] - lx) <= tol and abs(vals[1] - fx) <= tol, (tag, vals[0], lx, vals[1], fx)
                else:
                    for a, b_ in zip(_pattern(g_dev), _pattern(g_ref)):
                        assert np.array_equal(a, b_), tag
                    fin = np.isfinite(g_ref)
                    assert np.array_equal(g_dev[fin], g_ref[fin]), tag
                    assert not np.all(fin)
                    for a, b_ in ((vals[0], lx), (vals[1], fx)):
                        assert [bool(p) for p in _pattern(a)] == [bool(p) for p in _pattern(b_)], (tag, a, b_)
    finally:
        prob.close()


@pytest.mark.parametrize("dt", TYPES)
def test_stencil_refuses_rows_that_are_not_whole_packs(bz, dt):
    """A lane owns one 16-byte pack of a grid row: creation refuses ny % pack != 0 (2 fp64 / 4 fp32 elements)."""
    dtype = np.dtype(dt).type
    pk = 16 // np.dtype(dtype).itemsize
    for nx, ny in [(4, 1), (3, pk + 1), (2, 3 * pk - 1), (5, pk // 2 * 3)]:
        assert ny % pk
        n = nx * ny
        with pytest.raises(bz.BazingaHipError) as e:
            bz.Problem(bz.Stencil5ptQuadratic(nx, ny, np.zeros(n, dtype)), bz.Zero(), bz.IdentityFunction(), bz.FreeSet(),
                       n, n, dtype)
        assert e.value.code == bz._lib.BZ_ERR_ARG and "multiple of 16 bytes" in str(e.value), str(e.value)
    bz.Problem(bz.Stencil5ptQuadratic(3, 2 * pk, np.zeros(6 * pk, dtype)), bz.Zero(), bz.IdentityFunction(), bz.FreeSet(),
               6 * pk, 6 * pk, dtype).close()


# ------------------------------------------------------------------ (b) 30 states against the oracle
TRACE_GRID = (24, 32)
TRACE_STATES = 30
# l0box has a discontinuous prox (an entry is kept or zeroed), so it may stand here only while the oracle and its
# extended-precision twin stay together: they do, in every regime and both types (the docstring), so all 28 classes run
TRACE_CLASSES = CLASSES
TRACE_CASES = [(c, dt, regime, form) for dt in TYPES for c in TRACE_CLASSES for regime in ("uni0", uniform_regime(c))
               for form in (("default", "two-loop") if also_two_loop(c) else ("default",))]
TIGHT_STATES = {"float64": 25, "float32": 8}


def tight_states(envelope, dt):
    """how many states the comparison holds to its base tolerance, from the oracle's own sensitivity alone"""
    if dt == "float64":
        return sum(1 for s in envelope if iter_tol(s) == RTOL_ITER)
    return sum(1 for s in envelope if max(2e-5, 100 * s) <= 1e-3)


@pytest.mark.parametrize("cls,dt,regime,form", TRACE_CASES,
                         ids=["%s-%s-%s-%s" % (cid(c), d[-2:], r, f) for c, d, r, f in TRACE_CASES])
def test_stencil_iterates_follow_oracle(bz, ref, monkeypatch, cls, dt, regime, form):
    clear_knobs(monkeypatch)
    dtype = np.dtype(dt).type
    fp64 = dt == "float64"
    nx, ny = TRACE_GRID
    n = nx * ny
    dev, orc, mu, y, x0 = make_case(bz, ref, nx, ny, cls, dtype, regime)
    forms = []
    with np.errstate(all="ignore"):
        prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, TRACE_STATES, dtype=dtype,
                                    minimum_gamma=float(np.finfo(dtype).eps), compact=None if form == "default" else False,
                                    forms=forms, form_key="k_stencil_update")
    pr = prob.profile2()
    prob.close()
    # the fast path served the iterations, in the form asked for
    assert pr["k_stencil_fb"]["launches"] >= 20, pr["k_stencil_fb"]
    if form == "default":
        assert all(f.startswith("k_stencil_update_c<") for f in forms), sorted(set(forms))
        assert any("FULL=0" in f for f in forms) and any("FULL=1" in f for f in forms), sorted(set(forms))
    else:
        assert set(forms) == {"k_stencil_update"}, sorted(set(forms))
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        if fp64:
            assert abs(g_d - g_r) <= 1e-13 * g_r, (k, g_d, g_r)
            tol = iter_tol(sens)
            assert abs(sn_d - sn_r) <= 1e-8 * max(1.0, sn_r), (k, sn_d, sn_r)
        else:
            tol = max(2e-5, 100 * sens)
            if tol == 2e-5:
                assert abs(g_d - g_r) <= 1e-5 * g_r, (k, g_d, g_r)
        assert ex <= tol and ez <= tol, f"iterate mismatch at k={k}: {ex} {ez} (tol {tol})"
    # the widened tolerance may not carry the comparison
    tight = tight_states([r_[8] for r_ in rows], dt)
    assert tight >= TIGHT_STATES[dt], tight


# ------------------------------------------------------------------ (c) the fast passes against the generic chain
LOCKSTEP_GRID = (48, 64)
LOCKSTEP_STEPS = 40
MIN_TAU_RUNS, MIN_GAMMA_RUNS = 4, 8
_lockstep_counts = {}      # (class, type) -> [(regime, tau backtracks, gamma halvings) of the default form]


def lockstep_grid(cls):
    """the pinned grid of a class, alternating 1 and 8 workgroups: k_stencil_update_c runs on min(grid, BZ_SUC_GRID * CUs)
    workgroups, so a pin above the CU count would give it another summation tree than the generic kernels'"""
    return "1" if CLASSES.index(cls) % 2 == 0 else "8"


def _lockstep(bz, dev, shape, mu, y, x0, steps, members, dtype, monkeypatch):
    """Problems stepped side by side; members: (environment, fuse, compact).  Every state (x, z, res, the scalars, the
    counters) after every step, and the forms of the stencil launches seen."""
    nx, ny = shape
    n = nx * ny
    eps = float(np.finfo(dtype).eps)
    probs = []
    try:
        for env, fuse, compact in members:
            clear_knobs(monkeypatch, **env)
            prob = bz.Problem(*dev, n, n, dtype)
            probs.append(prob)
            prob.set_multipliers(mu, y)
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps, fuse=fuse,
                                          directions=bz.LBFGS(5, compact=compact)).c_opts(), x0)
        halvings0 = [prob.panoc_stats().n_gamma_halvings for prob in probs]      # (those of the start)
        runs = [[] for _ in members]
        seen = [set() for _ in members]
        for _ in range(steps):
            for prob, r, s in zip(probs, runs, seen):
                prob.panoc_step()
                st = prob.panoc_stats()
                r.append((prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_scalars(),
                          (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips)))
                p2 = prob.profile2()
                s.update(p2[k]["form"] for k in ("k_stencil_fb", "k_stencil_update") if p2[k]["launches"])
        return runs, seen, halvings0
    finally:
        for prob in probs:
            prob.close()


def _lockstep_class(bz, ref, monkeypatch, cls, dt):
    """Both runs of a class in one type; returns [(regime, tau backtracks, gamma halvings of the steps)] of the default
    form."""
    if (cls, dt) in _lockstep_counts:
        return _lockstep_counts[(cls, dt)]
    dtype = np.dtype(dt).type
    pin = {"BZ_GRID": lockstep_grid(cls)}
    out = []
    for regime, far in (("uni0", True), (uniform_regime(cls), False)):
        dev, orc, mu, y, x0 = make_case(bz, ref, *LOCKSTEP_GRID, cls, dtype, regime, far=far)
        compact_group = [(pin, True, True), (dict(pin, BZ_STENCIL_REGX="0"), True, True), (pin, False, True)]
        if regime != "uni0":
            compact_group.append((dict(pin, BZ_UNI="0"), True, True))      # (penalties streamed, not carried as numbers)
        two_loop_group = [(pin, True, False), (pin, False, False)]
        for group in (compact_group, two_loop_group):
            with np.errstate(all="ignore"):
                (base, *others), seen, halvings0 = _lockstep(bz, dev, LOCKSTEP_GRID, mu, y, x0, LOCKSTEP_STEPS, group, dtype,
                                                             monkeypatch)
            case = (cid(cls), dt, regime)
            assert np.all(np.isfinite(base[-1][0])), case      # (equal bits, and not because every run ended in NaN)
            for member, r in zip(group[1:], others):
                for k, (a, b_) in enumerate(zip(r, base)):
                    for u_, v_ in zip(a[:3], b_[:3]):
                        assert np.array_equal(u_, v_, equal_nan=True), (case, member, k + 1)
                    for key in SCALARS:
                        assert _same(a[3][key], b_[3][key]), (case, member, k + 1, key, a[3][key], b_[3][key])
                    assert a[4] == b_[4], (case, member, k + 1, a[4], b_[4])
            # the members ran what they stand for
            for (env, fuse, compact), s in zip(group, seen):
                if not fuse:
                    assert not s, (case, env, sorted(s))
                elif compact:
                    regx = env.get("BZ_STENCIL_REGX") != "0"
                    upd = [f for f in s if f.startswith("k_stencil_update")]
                    assert upd and all(f.startswith("k_stencil_update_c<") and ("REGX=1" in f) == regx for f in upd), \
                        (case, env, sorted(s))
                else:
                    assert "k_stencil_update" in s, (case, env, sorted(s))
            if group is compact_group:
                out.append((regime, base[-1][4][0], base[-1][4][1] - halvings0[0]))
    _lockstep_counts[(cls, dt)] = out
    return out


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("cls", CLASSES, ids=cid)
def test_stencil_fast_passes_equal_the_generic_chain(bz, ref, monkeypatch, cls, dt):
    """uni0 from the far start and the class's uniform regime from the near start: within the compact group (REGX = 1,
    REGX = 0, the generic chain, and in the uniform regime the penalties streamed) and within the two-loop group (fast
    passes, generic chain) x, z, res, the scalars and the counters are equal after every step."""
    _lockstep_class(bz, ref, monkeypatch, cls, dt)


@pytest.mark.parametrize("dt", TYPES)
def test_stencil_lockstep_walks_the_hard_paths(bz, ref, monkeypatch, dt):
    """Over the whole table of (c), from the device's own counters: runs with a tau backtrack, runs with a gamma halving.
    (The classes' runs are those of test_stencil_fast_passes_equal_the_generic_chain; a class not run yet in this process is
    run here.)"""
    runs = [r for cls in CLASSES for r in _lockstep_class(bz, ref, monkeypatch, cls, dt)]
    tau = sum(1 for _, nb, nh in runs if nb > 0)
    gam = sum(1 for _, nb, nh in runs if nh > 0)
    print(f"{dt}: {len(runs)} runs, {tau} with a tau backtrack, {gam} with a gamma halving")
    assert tau >= MIN_TAU_RUNS and gam >= MIN_GAMMA_RUNS, (tau, gam)


# ------------------------------------------------------------------ (d) the non-temporal instantiations
NT_GRIDS = {"float64": (2048, 2048), "float32": (2048, 3584)}      # n * sizeof(T) * 12 > 340e6 in both


@pytest.mark.parametrize("dt", TYPES)
def test_stencil_non_temporal_forms_are_bitwise_neutral(bz, monkeypatch, dt):
    """The obstacle problem with per-element penalties (the parameter streams go through the NTP loads), 12 steps as
    built and with BZ_XDNT=0: other instantiations of k_stencil_fb, k_compact_xd and k_stencil_update_c, the same bits.
    (No oracle at this size: the 2048^2 iterate test of test_gpu_parity holds the as-built form to it.)"""
    dtype = np.dtype(dt).type
    nx, ny = NT_GRIDS[dt]
    n = nx * ny
    assert n * np.dtype(dtype).itemsize * 12 > 340e6
    d = bz.synth.obstacle_grid(nx, ny, dtype=dtype, load=-1.0)
    dev = (bz.Stencil5ptQuadratic(nx, ny, d["b"]), bz.Zero(), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["psi"], np.inf)))
    rng = np.random.default_rng(zlib.crc32(("obstacle-%s" % dt).encode()))
    mu = (10.0 ** rng.uniform(-2, 0, n)).astype(dtype)
    y = (0.01 * rng.standard_normal(n)).astype(dtype)
    out = []
    for xdnt in (None, "0"):
        clear_knobs(monkeypatch, **({"BZ_XDNT": xdnt} if xdnt else {}))
        prob = bz.Problem(*dev, n, n, dtype)
        try:
            prob.set_multipliers(mu, y)
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(dtype).eps)).c_opts(), d["x0"])
            for _ in range(12):
                prob.panoc_step()
            p2 = prob.profile2()
            out.append((prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_scalars(),
                        [p2[k]["form"] for k in ("k_stencil_fb", "x_d", "k_stencil_update")]))
        finally:
            prob.close()
    (x1, z1, r1, s1, f1), (x2, z2, r2, s2, f2) = out
    assert f1 == ["k_stencil_fb<NT=1>", "k_compact_xd<FULL=1,NT=1>", "k_stencil_update_c<FULL=1,NT=1,REGX=1>"], f1
    assert f2 == ["k_stencil_fb<NT=0>", "k_compact_xd<FULL=1,NT=0>", "k_stencil_update_c<FULL=1,NT=0,REGX=1>"], f2
    assert np.array_equal(x1, x2, equal_nan=True) and np.array_equal(z1, z2, equal_nan=True)
    assert np.array_equal(r1, r2, equal_nan=True)
    for key in SCALARS:
        assert _same(s1[key], s2[key]), (key, s1[key], s2[key])
    assert np.all(np.isfinite(x1)) and s1["stop_norm"] > 0


# ------------------------------------------------------------------ (e) whole solves
def _oracle_solves(ref, orc, x0, y0):
    """ref.alps and its extended-precision twin (the resolution of the comparison)"""
    import warnings
    sub = lambda **kw: ref.PANOCplus(directions=ref.LBFGS(5, compact=True), **kw)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        o = ref.alps(*orc, x0, y0, maxit=40, subsolver=sub)
        ref.set_reducer(LongDoubleReducer())
        try:
            o2 = ref.alps(*orc, x0, y0, maxit=40, subsolver=sub)
        finally:
            ref.set_reducer(None)
    return o, o2


def solve_case(bz, ref, cls):
    nx, ny = TRACE_GRID
    dev, orc, mu, y, x0 = make_case(bz, ref, nx, ny, cls, np.float64, "uni1")
    return dev, orc, x0, 0.1 * y


@pytest.mark.parametrize("cls", CLASSES, ids=["%s-64" % cid(c) for c in CLASSES])
def test_stencil_alps_parity_over_the_table(bz, ref, monkeypatch, cls):
    """bz.alps, resident and through the host outer loop, against ref.alps (the compact form on both sides): the assertions
    of test_randomised_kinds_alps_parity.  f(x) alone (f_only) and the penalty probe of every AugLagUpdate! run here for
    every kind."""
    clear_knobs(monkeypatch)
    dev, orc, x0, y0 = solve_case(bz, ref, cls)
    o, o2 = _oracle_solves(ref, orc, x0, y0)
    a = bz.alps(*dev, x0, y0, maxit=40, resident=True)
    ah = bz.alps(*dev, x0, y0, maxit=40, resident=False)
    tag = f"{cid(cls)}: device {a[5]} outer {a[2]} inner {a[3]} | oracle {o[5]} outer {o[2]} inner {o[3]} | twin outer {o2[2]} inner {o2[3]}"
    print(tag)
    assert ah[2] == a[2] and ah[3] == a[3], (tag, ah[2], ah[3])      # resident and host outer loops: the same solve
    assert a[5] == o[5], tag
    assert a[2] == o[2] or o2[2] != o[2], tag
    assert abs(a[3] - o[3]) <= max(3, 0.3 * o[3]), tag
    scale = max(1.0, float(np.max(np.abs(o[0]))))
    self_x = float(np.max(np.abs(o2[0] - o[0])))
    tol = max((2e-5 if cls[1] in ("box", "box_vec") else 1e-6) * scale, 4.0 * self_x)
    err = np.abs(a[0] - o[0])
    if cls[0] == "l0box":       # the L0 prox is discontinuous: a tie may flip an entry (the oracle pair shows it too)
        frac_self = float(np.mean(np.abs(o2[0] - o[0]) <= 1e-4 * scale))
        assert np.mean(err <= max(tol, 1e-4 * scale)) >= min(0.999, frac_self - 0.002), tag
    else:
        assert np.max(err) <= tol, (tag, float(np.max(err)), tol)


# ------------------------------------------------------------------ the oracle-only figures of the docstring
def _oracle_pair(ref, orc, mu, y, x0, states, dtype, compact=False):
    """the oracle and its extended-precision twin: (envelope per state, tau backtracks, gamma halvings of the first)"""
    eps = float(np.finfo(dtype).eps)
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=eps,
                                    directions=ref.LBFGS(5, compact=compact))
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    env, envelope, tau, gam0 = 0.0, [], 0, sts[0].n_gamma_halvings      # (halvings of the steps, not of the start)
    for k in range(states):
        env = max(env, _err(sts[1].x, sts[0].x), _err(sts[1].z, sts[0].z))
        envelope.append(env)
        if k + 1 < states:
            sts[0] = its[0].step(sts[0])
            tau += sts[0].n_backtracks
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    return envelope, tau, sts[0].n_gamma_halvings - gam0


def oracle_only_figures(bz, ref):
    import warnings
    warnings.simplefilter("ignore")
    with np.errstate(all="ignore"):
        for dt in TYPES:
            dtype = np.dtype(dt).type
            worst = {}
            for cls in CLASSES:
                for regime in REGIMES:
                    dev, orc, mu, y, x0 = make_case(bz, ref, *TRACE_GRID, cls, dtype, regime)
                    envelope, _, _ = _oracle_pair(ref, orc, mu, y, x0, TRACE_STATES, dtype)
                    fig = (tight_states(envelope, dt), -envelope[-1], cid(cls), regime)
                    key = cls[0] == "l0box"
                    worst[key] = min(worst.get(key, fig), fig)
                    if fig[0] < TRACE_STATES:
                        print(f"(b) {dt} {cid(cls)} {regime}: {fig[0]} tight states, envelope {envelope[-1]:.2e}")
            for key, fig in sorted(worst.items()):
                print(f"(b) {dt} {'l0box' if key else 'without l0box'}: fewest tight states {fig[0]} ({fig[2]}, {fig[3]}), "
                      f"its envelope {-fig[1]:.2e}")
            tau_cls, gam_cls = [], []
            for cls in CLASSES:
                dev, orc, mu, y, x0 = make_case(bz, ref, *LOCKSTEP_GRID, cls, dtype, "uni0", far=True)
                _, tau, gam = _oracle_pair(ref, orc, mu, y, x0, LOCKSTEP_STEPS + 1, dtype)
                if tau:
                    tau_cls.append(cid(cls))
                if gam:
                    gam_cls.append(cid(cls))
            print(f"(c) {dt} far start: tau backtracks in {len(tau_cls)} of {len(CLASSES)} classes, gamma halvings in "
                  f"{len(gam_cls)}: {tau_cls} / {gam_cls}")


if __name__ == "__main__":
    import bazinga_jl_amd
    from oracle import bazinga_ref
    oracle_only_figures(bazinga_jl_amd, bazinga_ref)
