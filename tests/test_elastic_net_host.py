"""g = ElasticNet (BZ_G_ELASTIC_NET), host side: the numpy class against the closed-form prox in extended precision, the
subgradient condition, the value, the lowering into bz_problem_desc (g_lambda, g_l2, g_weights), the glmnet constructor,
refused arguments, the descriptor's two new fields and the Julia shim's methods.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_weighted_l1_host import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble

# (name, l1, l2, weighted): the number form, penalty factors with exact zeros, pure ridge, pure l1
FORMS = [("number", 0.7, 0.4, False), ("weighted", 0.7, 0.4, True), ("ridge", 0.0, 0.9, True), ("l2=0", 0.6, 0.0, True)]
GAMMAS = [3.7e-4, 2.1e-3, 0.037, 0.37, 5.3, 41.0]              # six decades


def form_of(bz, form, n, seed=0):
    """(the class, its weights or None); the weights are 2 * weights(n): U(0, 1) with the three exact zeros"""
    name, l1, l2, weighted = form
    w = 2.0 * weights(n, seed) if weighted else None
    return bz.ElasticNet(l1, l2, w), w


def exact_prox(y, gamma, l1, l2, w, dtype):
    """soft(y, gamma w l1) / (1 + gamma w l2) in np.longdouble, from the operands as the problem's type holds them;
    returns (z*, a) with a = gamma w l1"""
    T = np.dtype(dtype).type
    t = LD(T(gamma)) * (np.ones(y.shape, LD) if w is None else w.astype(dtype).astype(LD))
    a = t * LD(T(l1))
    yl = y.astype(LD)
    s = np.sign(yl) * np.maximum(np.abs(yl) - a, LD(0))
    return s / (LD(1) + t * LD(T(l2))), a


def prox_bound(y, a, dtype):
    """|z - z*| <= 8 eps (|y| + a) + the smallest normal.  The definition rounds seven times (t, a, t l2, d, s, the division
    and, inside s, the clamp's operand -a is exact): each rounding moves z by at most eps/2 (|y| + a) / d, d >= 1, and the
    one of d by as much again, so 8 eps covers them with room; below the smallest normal the roundings are absolute"""
    fi = np.finfo(dtype)
    return 8 * LD(fi.eps) * (np.abs(y.astype(LD)) + a) + LD(fi.tiny)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_prox_is_the_minimiser(bz, dtype, form):
    n = 200
    worst = 0.0
    for k, gamma in enumerate(GAMMAS):
        g, w = form_of(bz, form, n, k)
        rng = np.random.default_rng(100 + k)
        y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 2, n)).astype(dtype)
        z = np.empty(n, dtype)
        g.prox(z, y, gamma)
        assert z.dtype == dtype
        zs, a = exact_prox(y, gamma, g.l1, g.l2, w, dtype)
        err, bound = np.abs(z.astype(LD) - zs), prox_bound(y, a, dtype)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (gamma, float(np.max(err / bound)))
        if w is not None:                                        # a zero weight: wholly unpenalised
            assert np.array_equal(z[w == 0], y[w == 0])
    print(f"{form[0]} {np.dtype(dtype)}: worst |z - z*| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_subgradient_condition_at_z(bz, dtype, form):
    """(y - z) / gamma is in the subdifferential of g at z: equal to w (l1 sign z + l2 z) where z != 0, at most w l1 in size
    where z == 0; in longdouble, with the slack of the prox bound times (1 + gamma w l2)"""
    n = 200
    T = np.dtype(dtype).type
    moved = 0
    for k, gamma in enumerate(GAMMAS):
        g, w = form_of(bz, form, n, k)
        y = (np.random.default_rng(200 + k).standard_normal(n) * 3.0).astype(dtype)
        z = np.empty(n, dtype)
        g.prox(z, y, gamma)
        t = LD(T(gamma)) * (np.ones(n, LD) if w is None else w.astype(dtype).astype(LD))
        a, d = t * LD(T(g.l1)), LD(1) + t * LD(T(g.l2))
        zl, yl = z.astype(LD), y.astype(LD)
        slack = prox_bound(y, a, dtype) * d
        nz = zl != 0
        assert np.all(np.abs(yl - zl - (a * np.sign(zl) + (d - 1) * zl))[nz] <= slack[nz])
        assert np.all(np.abs(yl)[~nz] <= a[~nz] + slack[~nz])
        moved += int(nz.sum())
    assert moved >= n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_call_is_the_sum_of_the_terms(bz, dtype):
    n = 64
    x = np.random.default_rng(3).standard_normal(n).astype(dtype)
    for form in FORMS:
        g, w = form_of(bz, form, n, 5)
        ww = np.ones(n) if w is None else w
        terms = [ww[i] * (g.l1 * abs(float(x[i])) + 0.5 * g.l2 * float(x[i]) ** 2) for i in range(n)]
        assert abs(float(g(x)) - sum(terms)) <= 64 * np.finfo(dtype).eps * sum(terms)
        # ... and what prox returns is g at the z it wrote
        z = np.empty(n, dtype)
        v = g.prox(z, x, 0.37)
        assert abs(float(v) - float(g(z.astype(np.float64)))) <= 64 * np.finfo(dtype).eps * float(g(z.astype(np.float64)))
    assert float(bz.ElasticNet(0.5, 0.25)(np.array([2.0, -4.0]))) == 0.5 * 6.0 + 0.125 * 20.0


def test_specials_go_through_the_definition(bz):
    """NaN stays NaN, an infinity keeps its sign, zeros of either sign and y = +-a give +0 (the operations of the
    definition: y - y and a - a are +0, and +0 / d is +0)"""
    g = bz.ElasticNet(0.5, 0.25)
    a = 0.37 * 0.5
    y = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, a, -a, 2.0])
    z = np.empty(8)
    with np.errstate(invalid="ignore"):
        g.prox(z, y, 0.37)
    assert np.isnan(z[0]) and z[1] == np.inf and z[2] == -np.inf
    assert np.all(z[3:7] == 0) and not np.signbit(z[3:7]).any()
    assert z[7] == (2.0 - a) / (1 + 0.37 * 0.25)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lowering_fills_the_descriptor(bz, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    n = 9
    w = 2.0 * weights(n, 3)
    rest = (bz.IdentityFunction(), bz.FreeSet())
    desc, keep = lower(bz.Zero(), bz.ElasticNet(0.75, 0.25, w), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == L.BZ_G_ELASTIC_NET == 11 and desc.g_lambda == 0.75 and desc.g_l2 == 0.25 and desc.g_weights
    assert not desc.g_lambda_vec
    held = [a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == desc.g_weights]
    assert len(held) == 1 and held[0].dtype == dtype and np.array_equal(held[0], w.astype(dtype))      # (kept alive)
    desc, keep = lower(bz.Zero(), bz.ElasticNet(0.75, 0.25), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == 11 and desc.g_lambda == 0.75 and desc.g_l2 == 0.25 and not desc.g_weights
    with pytest.raises(ValueError):
        lower(bz.Zero(), bz.ElasticNet(0.75, 0.25, w[:-1]), *rest, n, n, np.dtype(dtype))
    # the slack form: n entries, the x half
    desc, keep = lower(bz.Zero(), bz.ElasticNet(0.75, 0.25, w[:8]), *rest, 8, 8, np.dtype(dtype), True)
    assert desc.g_weights and desc.slack == 1
    # every other kind leaves the two fields zero
    desc, keep = lower(bz.Zero(), bz.NormL1(0.5), *rest, n, n, np.dtype(dtype))
    assert desc.g_l2 == 0.0 and not desc.g_weights


def test_numbers_that_overflow_the_problems_type_are_refused(bz):
    from bazinga_jl_amd.oracles import lower
    rest = (bz.IdentityFunction(), bz.FreeSet())
    for g in (bz.ElasticNet(1e39, 0.5), bz.ElasticNet(0.5, 1e39)):
        lower(bz.Zero(), g, *rest, 4, 4, np.dtype(np.float64))
        with pytest.raises(ValueError):
            lower(bz.Zero(), g, *rest, 4, 4, np.dtype(np.float32))


def test_glmnet_gives_the_two_products(bz):
    pf = np.array([0.0, 1.0, 2.5])
    g = bz.ElasticNet.glmnet(0.8, 0.25, pf)
    assert isinstance(g, bz.ElasticNet) and g.l1 == 0.8 * 0.25 and g.l2 == 0.8 * (1 - 0.25) and np.array_equal(g.weights, pf)
    pf[1] = 9.0
    assert g.weights[1] == 1.0                                   # (its own copy)
    g = bz.ElasticNet.glmnet(0.8, 1.0)
    assert (g.l1, g.l2, g.weights) == (0.8, 0.0, None)
    g = bz.ElasticNet.glmnet(0.8, 0.0)
    assert (g.l1, g.l2) == (0.0, 0.8)
    for alpha in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            bz.ElasticNet.glmnet(0.8, alpha)
    d = bz.ElasticNet()
    assert (d.l1, d.l2, d.weights) == (1.0, 1.0, None)


def test_bad_arguments_raise(bz):
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            bz.ElasticNet(bad, 0.5)
        with pytest.raises(ValueError):
            bz.ElasticNet(0.5, bad)
        with pytest.raises(ValueError):
            bz.ElasticNet(0.5, 0.5, np.array([0.1, bad, 0.3]))
    with pytest.raises(ValueError):
        bz.ElasticNet(np.array([0.5, 0.5]), 0.5)
    with pytest.raises(ValueError):
        bz.ElasticNet(0.5, 0.5, np.ones((2, 3)))
    with pytest.raises(ValueError):
        bz.ElasticNet.glmnet(-1.0, 0.5)


def test_the_two_fields_sit_behind_g_hi(bz):
    """in the g block, between g_hi and g_lo_vec: the neighbourhoods that the other host tests pin (the last nine fields among
    them) stay as they are"""
    L = bz._lib
    names = [f for f, _ in L.ProblemDesc._fields_]
    i = names.index("g_l2")
    assert names[i - 1:i + 3] == ["g_hi", "g_l2", "g_weights", "g_lo_vec"]
    assert dict(L.ProblemDesc._fields_)["g_l2"] is C.c_double and dict(L.ProblemDesc._fields_)["g_weights"] is C.c_void_p
    assert L.ProblemDesc.g_l2.offset == L.ProblemDesc.g_hi.offset + 8 and L.ProblemDesc.g_weights.offset == L.ProblemDesc.g_hi.offset + 16
    assert L.SIGNATURES["bz_problem_set_g_elastic_net"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double])
    assert hasattr(bz.Problem, "set_g_elastic_net")
    header = open(os.path.join(ROOT, "include", "bazinga_hip.h")).read()
    assert re.search(r"#define BZ_G_ELASTIC_NET\s+11\b", header)
    assert re.search(r"double\s+g_lo, g_hi;[^\n]*\n\s*double\s+g_l2;[^\n]*\n[^\n;]*\n\s*const void\*\s+g_weights;", header)
    assert "int bz_problem_set_g_elastic_net(bz_problem* p, double l1, double l2);" in header


def test_julia_shim_names_the_type():
    src = open(os.path.join(ROOT, "julia", "BazingaHIP.jl")).read()
    assert re.search(r"^struct ElasticNet\{W", src, re.M)
    assert re.search(r"lower_g!\(d, g::ElasticNet\{Nothing\}\) = \(d\.g_kind = 11; d\.g_lambda = g\.l1; d\.g_l2 = g\.l2\)", src)
    assert re.search(r"lower_g!\(d, g::ElasticNet\{<:AbstractVector\}\) = \(d\.g_kind = 11; d\.g_lambda = g\.l1; d\.g_l2 = g\.l2; "
                     r"d\.g_weights = pointer\(g\.weights\)\)", src)
    assert re.search(r"lower_g!\(d, g::ProximalOperators\.ElasticNet\{<:Real,<:Real\}\) = \(d\.g_kind = 11; d\.g_lambda = g\.mu; "
                     r"d\.g_l2 = g\.lambda\)", src)
    assert re.search(r"set_g_elastic_net!\(p::Problem, l1::Real, l2::Real\) = check\(ccall\(\(:bz_problem_set_g_elastic_net, lib\)", src)
    assert re.search(r"g_l2::Float64 = 0; g_weights::Ptr\{Cvoid\} = C_NULL", src)
