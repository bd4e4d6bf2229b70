"""NormL21 (the group Lasso over contiguous blocks of K elements), host side: the numpy class that specifies the device
kernel against a plain per-group loop with the same fold, its edge cases, the lowering into bz_problem_desc (kind 9, g_group
directly behind g_p, lambda as a number or one entry per group) and the Julia shim.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 3, 5, 8, 33, 64]


def loop_prox(y, lam, K, gamma):
    """the definition, one group at a time, scalars of y's type throughout; returns (z, the groups' terms scal * nrm)"""
    T = y.dtype.type
    ng = y.shape[0] // K
    KP = 1
    while KP < K:
        KP *= 2
    z = np.empty_like(y)
    terms = np.empty(ng, y.dtype)
    with np.errstate(all="ignore"):
        for j in range(ng):
            yj = y[j * K:(j + 1) * K]
            q = [T(0)] * KP
            for k in range(K):
                q[k] = yj[k] * yj[k]
            o = KP // 2
            while o >= 1:
                for i in range(o):
                    q[i] = q[i] + q[i + o]
                o //= 2
            nrm = np.sqrt(q[0])
            gl = T(gamma) * T(lam[j] if np.ndim(lam) else lam)
            if nrm <= gl:
                scal = T(0)
                z[j * K:(j + 1) * K] = T(0)
            else:
                scal = T(1) - gl / nrm if nrm > gl else nrm - gl
                for k in range(K):
                    z[j * K + k] = scal * yj[k]
            terms[j] = scal * nrm
    return z, terms


def group_weights(ng, seed=0):
    lam = 0.6 * np.random.default_rng(seed).uniform(0.2, 1.0, ng)
    lam[0] = 0.0
    if ng > 2:
        lam[ng // 2] = 0.0
    return lam


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", KS)
def test_prox_equals_the_per_group_loop_bit_for_bit(bz, K, dtype):
    ng, gamma = 23, 0.37
    rng = np.random.default_rng(100 + K)
    y = rng.standard_normal(ng * K).astype(dtype)
    y[K:2 * K] *= dtype(0.01)                                # a group that the penalty zeroes
    y[2 * K:3 * K] = 0                                       # a zero group
    for lam in (0.8, group_weights(ng, K)):
        g = bz.NormL21(lam, K)
        z = np.empty_like(y)
        v = g.prox(z, y, gamma)
        zl, terms = loop_prox(y, np.asarray(lam, dtype) if np.ndim(lam) else lam, K, gamma)
        assert z.dtype == dtype and np.array_equal(z.view(np.uint8), zl.view(np.uint8))
        assert np.all(z[K:2 * K] == 0) or np.ndim(lam)
        want = np.sum(np.asarray(lam, dtype) * terms) if np.ndim(lam) else dtype(lam) * np.sum(terms)
        assert v == want and type(v) is type(want) and np.isfinite(v)
        # g(z) itself, to rounding
        ref_val = np.sum(np.asarray(lam, np.float64) * np.sqrt(np.sum(z.astype(np.float64).reshape(ng, K) ** 2, axis=1)))
        assert abs(float(v) - ref_val) <= 64 * np.finfo(dtype).eps * max(1.0, ref_val)
        assert abs(float(g(z)) - ref_val) <= 64 * np.finfo(dtype).eps * max(1.0, ref_val)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_threshold_zero_lambda_nan_and_inf(bz, dtype):
    K, gamma = 4, 0.5
    T = dtype
    # ||y|| <= gamma lambda: exactly zero, the threshold included (3-4-0-0 has the exact norm 5)
    y = np.array([3, 4, 0, 0, 0.3, -0.4, 0, 0, 3, 4, 0, 0.5], T)
    g = bz.NormL21(10.0, K)                                  # gl = 5
    z = np.full_like(y, 7)
    v = g.prox(z, y, gamma)
    assert np.all(z[:8] == 0) and not np.any(np.signbit(z[:8])) and np.all(z[[8, 9, 11]] != 0) and z[10] == 0 and v > 0
    # lambda = 0: y bit for bit, a zero group (0 / 0 in the quotient form) and signed zeros included
    y = np.array([1.5, -2.0, 0.0, -0.0, 0.0, 0.0, 0.0, 0.0, -0.0, 2.5, 0.0, 0.0], T)
    for lam in (0.0, np.zeros(3)):
        z = np.full_like(y, 7)
        v = bz.NormL21(lam, K).prox(z, y, gamma)
        assert np.array_equal(z.view(np.uint8), y.view(np.uint8)) and v == 0
    # a NaN poisons its own group and nothing else; an infinite element gives z = y
    y = np.arange(1, 17, dtype=T)
    y[7] = np.nan
    y[9] = np.inf
    y[14] = -np.inf
    lam = np.array([0.5, 0.5, 0.25, 2.0])
    z = np.empty_like(y)
    with np.errstate(invalid="ignore"):
        v = bz.NormL21(lam, K).prox(z, y, gamma)
    assert np.all(np.isnan(z[4:8])) and not np.any(np.isnan(z[:4])) and np.isnan(v)
    assert np.array_equal(z[8:16], y[8:16])
    y[7] = 8
    with np.errstate(invalid="ignore"):
        v = bz.NormL21(lam, K).prox(z, y, gamma)
    assert np.isinf(v) and v > 0 and np.all(np.isfinite(z[:8]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_group_of_one_is_the_l1_norm(bz, dtype):
    n, gamma = 40, 0.3
    y = np.random.default_rng(5).standard_normal(n).astype(dtype)
    lam = group_weights(n, 6)
    for lm in (0.7, lam):
        z1, z2 = np.empty_like(y), np.empty_like(y)
        v1, v2 = bz.NormL1(lm).prox(z1, y, gamma), bz.NormL21(lm, 1).prox(z2, y, gamma)
        eps = np.finfo(dtype).eps
        assert np.all(np.abs(z1 - z2) <= 4 * eps * np.abs(y)) and np.array_equal(z1 == 0, z2 == 0)
        assert abs(float(v1) - float(v2)) <= 8 * n * eps * max(1.0, abs(float(v1)))


@pytest.mark.parametrize("K", [1, 3, 8])
def test_prox_point_minimises_the_prox_objective(bz, K):
    ng, gamma = 6, 0.8
    rng = np.random.default_rng(7 + K)
    y = rng.standard_normal(ng * K)
    y[K:2 * K] *= 0.05                                       # (a group the penalty zeroes)
    lam = group_weights(ng, 8)
    g = bz.NormL21(lam, K)
    z = np.empty_like(y)
    g.prox(z, y, gamma)

    def obj(w):
        return float(g(w)) + np.sum((w - y) ** 2) / (2 * gamma)
    base = obj(z)
    assert np.all(z[K:2 * K] == 0) and np.all(z[:K] == y[:K])
    for t in range(50):
        w = z + 10.0 ** rng.uniform(-6, 0) * rng.standard_normal(ng * K)
        assert base <= obj(w)


def test_constructor_refuses_bad_arguments(bz):
    g = bz.NormL21(np.array([0.0, 1.0]), 3)
    assert g.group == 3 and isinstance(g.lam, np.ndarray) and type(bz.NormL21(0.5, 2).lam) is float
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            bz.NormL21(1.0, bad)
    for bad in (-1.0, np.nan, np.inf, np.array([0.1, -0.1]), np.array([np.nan]), np.ones((2, 2))):
        with pytest.raises(ValueError):
            bz.NormL21(bad, 2)
    with pytest.raises(ValueError):
        bz.NormL21(1.0, 4).prox(np.empty(6), np.ones(6), 1.0)
    with pytest.raises(ValueError):
        bz.NormL21(np.ones(2), 2).prox(np.empty(6), np.ones(6), 1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_sets_kind_group_and_lambda(bz, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    K, ng = 3, 5
    n = K * ng
    rest = (bz.IdentityFunction(), bz.FreeSet())
    desc, keep = lower(bz.Zero(), bz.NormL21(0.25, K), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == L.BZ_G_NORM_L21 == 9 and desc.g_group == K and desc.g_lambda == 0.25 and not desc.g_lambda_vec
    lam = group_weights(ng, 2)
    desc, keep = lower(bz.Zero(), bz.NormL21(lam, K), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == 9 and desc.g_group == K and desc.g_lambda_vec
    held = [a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == desc.g_lambda_vec]
    assert len(held) == 1 and held[0].dtype == dtype and np.array_equal(held[0], lam.astype(dtype))      # (kept alive)
    # the other kinds leave g_group zero
    desc, keep = lower(bz.Zero(), bz.NormL1(0.25), *rest, n, n, np.dtype(dtype))
    assert desc.g_group == 0
    # refused before any device call: a length that is no multiple of the group, a vector of the wrong length, the slack form
    with pytest.raises(ValueError, match="multiple"):
        lower(bz.Zero(), bz.NormL21(0.25, K), *rest, n + 1, n + 1, np.dtype(dtype))
    with pytest.raises(ValueError):
        lower(bz.Zero(), bz.NormL21(lam[:-1], K), *rest, n, n, np.dtype(dtype))
    with pytest.raises(bz.UnsupportedOracle, match="slack"):
        lower(bz.Zero(), bz.NormL21(0.25, 2), *rest, 8, 8, np.dtype(dtype), True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.NormL21(0.25, 2), *rest, 8, 8, np.dtype(dtype), slack=True)


def test_field_sits_directly_behind_g_p_and_the_pinned_neighbourhoods_stay(bz):
    L = bz._lib
    names = [f for f, _ in L.ProblemDesc._fields_]
    i = names.index("g_group")
    assert names[i - 1] == "g_p" and names[i + 1] == "g_u"
    assert L.ProblemDesc.g_group.offset == L.ProblemDesc.g_p.offset + 8 and L.ProblemDesc.g_group.size == 8
    assert dict(L.ProblemDesc._fields_)["g_group"] is C.c_int64
    assert names[names.index("f_rows") + 1] == "f_classes" and names[names.index("f_classes") + 1] == "g_lambda"
    assert names[names.index("g_lambda_vec") - 1] == "g_hi_vec" and names[names.index("g_lambda_vec") + 1] == "c_A"
    assert names[-9:] == ["f_sp_nnz", "f_loss", "f_loss_delta", "f_w", "f_scale", "c_sp_rowptr", "c_sp_col", "c_sp_val", "c_sp_nnz"]
    assert L.BZ_G_CALLBACK == 8 and L.BZ_G_NORM_LP_BOX == 7
    header = open(os.path.join(ROOT, "include", "bazinga_hip.h")).read()
    assert re.search(r"#define BZ_G_NORM_L21\s+9\b", header)
    assert re.search(r"double\s+g_p;[^\n]*\n\s*int64_t\s+g_group;", header)


def test_a_foreign_f_sends_all_four_kinds_to_callbacks(bz):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib

    class MyF:
        def gradient(self, dfx, x):
            dfx[...] = x
            return 0.5 * float(x @ x)
    desc, keep = lower(MyF(), bz.NormL21(0.5, 2), bz.IdentityFunction(), bz.FreeSet(), 8, 8, np.float64)
    assert (desc.f_kind, desc.g_kind, desc.c_kind, desc.D_kind) == (L.BZ_F_CALLBACK, L.BZ_G_CALLBACK, L.BZ_C_CALLBACK, L.BZ_D_CALLBACK)
    # ... where the numpy class is the prox the library calls back
    x = np.array([3.0, 4.0, 0.1, 0.1, 0, 0, 1, 0])
    z = (C.c_double * 8)()
    xb = (C.c_double * 8)(*x)
    v = desc.cb_g_prox(None, C.addressof(xb), 1.0, C.addressof(z), 8)
    want = np.empty(8)
    wv = bz.NormL21(0.5, 2).prox(want, x, 1.0)
    assert np.array_equal(np.array(z), want) and v == wv and want[2] == 0 and want[0] == 3.0 * (1 - 0.5 / 5.0)


def test_julia_shim_names_the_type():
    src = open(os.path.join(ROOT, "julia", "BazingaHIP.jl")).read()
    assert re.search(r"struct NormL21\b", src)
    assert re.search(r"lower_g!\(d, g::NormL21\{<:Real\}\) = \(d\.g_kind = 9; d\.g_group = g\.group; d\.g_lambda = g\.lambda\)", src)
    assert re.search(r"lower_g!\(d, g::NormL21\{<:AbstractVector\}\) = \(d\.g_kind = 9; d\.g_group = g\.group; d\.g_lambda_vec = pointer", src)
    m = re.search(r"mutable struct ProblemDesc\n(.*?)\nend", src, re.S)
    assert re.search(r"g_p::Float64 = 0; g_group::Int64 = 0; g_u::", m.group(1))
