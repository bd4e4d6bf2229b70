"""GroupLasso (the group Lasso over a group pointer, with an optional l1 mix), host side: the numpy class that specifies the
device kernel — a minimiser of its prox objective, equal to a plain per-group loop over the 64 accumulators, and bit for bit
NormL21 where the sizes are equal — its constructor errors, the lowering into bz_problem_desc (kind 10, g_group_ptr /
g_ngroups / g_l1 directly behind g_u) and the Julia shim.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 3, 5, 8, 33, 64]
MIXED = [1, 2, 3, 5, 8, 13, 1, 40, 63, 64, 65, 127, 128, 129, 1, 200, 2, 1000]


def soft(y, t):
    """the threshold of one element, as the class states it"""
    T = type(y)
    if y > t:
        return y - t
    if y < -t:
        return y + t
    return y if np.isnan(y) else T(0)


def acc_sum(v):
    """64 accumulators a[p] = v[p] + v[p + 64] + ... in that order, then a[:o] + a[o:2o] for o = 32 .. 1"""
    T = v.dtype.type
    a = [None] * 64
    for k in range(v.shape[0]):
        a[k % 64] = v[k] if a[k % 64] is None else a[k % 64] + v[k]
    a = [T(0) if e is None else e for e in a]
    o = 32
    while o >= 1:
        for i in range(o):
            a[i] = a[i] + a[i + o]
        o //= 2
    return a[0]


def loop_prox(y, lam, ptr, l1, gamma):
    """the definition, one group at a time, scalars of y's type throughout; returns (z, the value)"""
    T = y.dtype.type
    z = np.empty_like(y)
    terms = []
    with np.errstate(all="ignore"):
        t = T(gamma) * T(l1)
        for j in range(len(ptr) - 1):
            yj = y[ptr[j]:ptr[j + 1]]
            u = np.array([soft(v, t) for v in yj], y.dtype) if l1 > 0 else yj
            nrm = np.sqrt(acc_sum(u * u))
            lj = T(lam[j] if np.ndim(lam) else lam)
            gl = T(gamma) * lj
            if nrm <= gl:
                scal = T(0)
                z[ptr[j]:ptr[j + 1]] = T(0)
            else:
                scal = T(1) - gl / nrm if nrm > gl else nrm - gl
                z[ptr[j]:ptr[j + 1]] = scal * u
            if l1 > 0:
                terms.append(lj * (scal * nrm) + (T(l1) * scal) * acc_sum(np.abs(u)))
            else:
                terms.append((lj * (scal * nrm)) if np.ndim(lam) else scal * nrm)
        terms = np.array(terms, y.dtype)
        if l1 > 0 or np.ndim(lam):
            return z, np.sum(terms)
        return z, T(lam) * np.sum(terms)


def group_weights(ng, seed=0):
    lam = 0.6 * np.random.default_rng(seed).uniform(0.2, 1.0, ng)
    lam[0] = 0.0
    if ng > 2:
        lam[ng // 2] = 0.0
    return lam


@pytest.mark.parametrize("l1", [0.0, 0.3])
@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
def test_prox_point_minimises_the_prox_objective(bz, vector, l1):
    sizes = [1, 3, 8, 2, 70, 5]
    ng, n, gamma = len(sizes), sum(sizes), 0.8
    rng = np.random.default_rng(7)
    y = rng.standard_normal(n)
    y[1:4] *= 0.05                                           # (a group the penalty zeroes)
    lam = group_weights(ng, 8) if vector else 0.45
    g = bz.GroupLasso.from_sizes(lam, sizes, l1)
    z = np.empty_like(y)
    v = g.prox(z, y, gamma)
    assert abs(float(v) - float(g(z))) <= 1e-12 * max(1.0, float(g(z)))

    def obj(w):
        return float(g(w)) + np.sum((w - y) ** 2) / (2 * gamma)
    base = obj(z)
    assert vector or np.all(z[1:4] == 0)
    assert np.any(z != 0) and (l1 == 0 or np.any(z[12:] == 0))
    for t in range(50):
        w = z + 10.0 ** rng.uniform(-6, 0) * rng.standard_normal(n)
        assert base <= obj(w)


@pytest.mark.parametrize("l1", [0.0, 0.3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prox_equals_the_per_group_loop_bit_for_bit(bz, dtype, l1):
    gamma = 0.37
    ptr = np.concatenate(([0], np.cumsum(MIXED)))
    rng = np.random.default_rng(100)
    y = rng.standard_normal(ptr[-1]).astype(dtype)
    y[1:3] *= dtype(0.01)                                    # a group that the penalty zeroes
    y[3:6] = 0                                               # a zero group
    for lam in (0.8, group_weights(len(MIXED), 3)):
        g = bz.GroupLasso(lam, ptr, l1)
        z = np.empty_like(y)
        v = g.prox(z, y, gamma)
        zl, vl = loop_prox(y, np.asarray(lam, dtype) if np.ndim(lam) else lam, ptr, l1, gamma)
        assert z.dtype == dtype and np.array_equal(z.view(np.uint8), zl.view(np.uint8))
        assert v == vl and type(v) is type(vl) and np.isfinite(v)
        ref_val = float(g(z.astype(np.float64)))
        assert abs(float(v) - ref_val) <= 64 * np.finfo(dtype).eps * max(1.0, ref_val)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_group_sums_follow_the_accumulator_order(bz, dtype):
    """every size in 1 .. 64 and around every multiple of 64 up to 4097, against the plain loop"""
    sizes = list(range(1, 67)) + [127, 128, 129, 191, 192, 193, 1000, 4095, 4096, 4097]
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    q = np.random.default_rng(5).standard_normal(ptr[-1]).astype(dtype) ** 2
    s = bz.GroupLasso(1.0, ptr).group_sums(q)
    want = np.array([acc_sum(q[ptr[j]:ptr[j + 1]]) for j in range(len(sizes))], dtype)
    assert s.dtype == dtype and np.array_equal(s, want)
    # (the order matters at these sizes: a plain left-to-right sum differs somewhere)
    plain = np.array([np.cumsum(q[ptr[j]:ptr[j + 1]])[-1] for j in range(len(sizes))], dtype)
    assert not np.array_equal(s, plain)


@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equal_sizes_are_norm_l21_bit_for_bit(bz, dtype, K, vector):
    ng, gamma = 23, 0.37
    rng = np.random.default_rng(100 + K)
    y = rng.standard_normal(ng * K).astype(dtype)
    y[K:2 * K] *= dtype(0.01)
    y[2 * K:3 * K] = 0
    y[3 * K] = -0.0
    lam = group_weights(ng, K) if vector else 0.8
    z1, z2 = np.empty_like(y), np.empty_like(y)
    v1 = bz.NormL21(lam, K).prox(z1, y, gamma)
    v2 = bz.GroupLasso.from_sizes(lam, [K] * ng).prox(z2, y, gamma)
    assert np.array_equal(z1.view(np.uint8), z2.view(np.uint8)) and v1 == v2 and type(v1) is type(v2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ties_signed_zeros_and_nan(bz, dtype):
    T = dtype
    gamma = T(0.5)
    t = gamma * T(0.5)                                       # 0.25, exact
    y = np.array([t, -t, 0.0, -0.0, 2.0, -2.0, np.nan, 1.0, 0.1, -0.1], T)
    g = bz.GroupLasso(0.0, [0, 4, 6, 8, 10], l1=0.5)
    z = np.full_like(y, 7)
    with np.errstate(invalid="ignore"):
        g.prox(z, y, gamma)
    # the ties and both zeros give +0; a NaN poisons its own group and nothing else
    assert np.all(z[:4] == 0) and not np.any(np.signbit(z[:4]))
    assert z[4] == T(1.75) and z[5] == T(-1.75)
    assert np.all(np.isnan(z[6:8])) and np.all(z[8:] == 0) and not np.any(np.signbit(z[8:]))
    # l1 == 0 and lambda == 0: y bit for bit, -0 included (the threshold is not evaluated)
    y = np.array([1.5, -0.0, 0.0, -2.0, -0.0], T)
    z = np.full_like(y, 7)
    v = bz.GroupLasso(0.0, [0, 2, 5]).prox(z, y, gamma)
    assert np.array_equal(z.view(np.uint8), y.view(np.uint8)) and v == 0


def test_constructor_refuses_bad_arguments(bz):
    g = bz.GroupLasso(np.array([0.0, 1.0]), [0, 3, 4], l1=0.25)
    assert g.ngroups == 2 and g.indptr.dtype == np.int64 and isinstance(g.lam, np.ndarray) and g.l1 == 0.25
    assert type(bz.GroupLasso(0.5, [0, 2]).lam) is float and bz.GroupLasso(0.5, [0, 2]).l1 == 0.0
    assert np.array_equal(bz.GroupLasso.from_sizes(1.0, [3, 1, 17]).indptr, [0, 3, 4, 21])
    bad_ptrs = ([1, 3, 4],                 # not starting at 0
                [0, 3, 3, 5],              # an empty group
                [0, 3, 2, 5],              # decreasing
                [0.0, 2.0, 4.0],           # not integers
                [0], [[0, 1], [1, 2]], [True, True])
    for bad in bad_ptrs:
        with pytest.raises(ValueError):
            bz.GroupLasso(1.0, bad)
    for bad in ([0, 2], [2.0, 1.0], [], [[1, 2]]):
        with pytest.raises(ValueError):
            bz.GroupLasso.from_sizes(1.0, bad)
    for bad in (-1.0, np.nan, np.inf, np.array([0.1, -0.1]), np.array([np.nan, 1.0]), np.ones((2, 2)), np.ones(3)):
        with pytest.raises(ValueError):
            bz.GroupLasso(bad, [0, 2, 4])
    for bad in (-0.1, np.nan, np.inf, np.ones(2), True):
        with pytest.raises(ValueError):
            bz.GroupLasso(1.0, [0, 2, 4], l1=bad)
    with pytest.raises(ValueError):
        bz.GroupLasso(1.0, [0, 2, 4]).prox(np.empty(6), np.ones(6), 1.0)
    with pytest.raises(ValueError):
        bz.GroupLasso(1.0, [0, 2, 4])(np.ones(5))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_sets_kind_pointer_and_l1(bz, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    sizes = [3, 1, 17, 70]
    n, ng = sum(sizes), len(sizes)
    rest = (bz.IdentityFunction(), bz.FreeSet())
    g = bz.GroupLasso.from_sizes(0.25, sizes, l1=0.125)
    desc, keep = lower(bz.Zero(), g, *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == L.BZ_G_GROUP_LASSO == 10 and desc.g_ngroups == ng and desc.g_l1 == 0.125
    assert desc.g_lambda == 0.25 and not desc.g_lambda_vec and desc.g_group == 0
    held = [a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == desc.g_group_ptr]
    assert len(held) == 1 and held[0].dtype == np.int64 and np.array_equal(held[0], [0, 3, 4, 21, 91])      # (kept alive)
    lam = group_weights(ng, 2)
    desc, keep = lower(bz.Zero(), bz.GroupLasso.from_sizes(lam, sizes), *rest, n, n, np.dtype(dtype))
    assert desc.g_kind == 10 and desc.g_lambda_vec and desc.g_group_ptr and desc.g_l1 == 0.0
    held = [a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == desc.g_lambda_vec]
    assert len(held) == 1 and held[0].dtype == dtype and np.array_equal(held[0], lam.astype(dtype))
    # the other kinds leave the three fields zero
    for other in (bz.NormL1(0.25), bz.NormL21(0.25, 1), bz.Zero()):
        desc, keep = lower(bz.Zero(), other, *rest, n, n, np.dtype(dtype))
        assert not desc.g_group_ptr and desc.g_ngroups == 0 and desc.g_l1 == 0.0
    # refused before any device call: a pointer that does not end at n, the slack form, a split-layout pairwise set
    with pytest.raises(ValueError, match="indptr"):
        lower(bz.Zero(), g, *rest, n + 1, n + 1, np.dtype(dtype))
    with pytest.raises(bz.UnsupportedOracle, match="slack"):
        lower(bz.Zero(), bz.GroupLasso(0.25, [0, 2, 8]), *rest, 8, 8, np.dtype(dtype), True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.GroupLasso(0.25, [0, 2, 8]), *rest, 8, 8, np.dtype(dtype), slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="split"):
        lower(bz.Zero(), bz.GroupLasso(0.25, [0, 2, 8]), bz.IdentityFunction(), bz.PairwiseSet("xor", layout="split"), 8, 8, np.dtype(dtype))


def test_fields_sit_directly_behind_g_u_and_the_pinned_neighbourhoods_stay(bz):
    L = bz._lib
    names = [f for f, _ in L.ProblemDesc._fields_]
    i = names.index("g_u")
    assert names[i - 2:i + 5] == ["g_p", "g_group", "g_u", "g_group_ptr", "g_ngroups", "g_l1", "g_lo"]
    types = dict(L.ProblemDesc._fields_)
    assert types["g_group_ptr"] is C.c_void_p and types["g_ngroups"] is C.c_int64 and types["g_l1"] is C.c_double
    assert L.ProblemDesc.g_group_ptr.offset == L.ProblemDesc.g_u.offset + 8
    assert L.ProblemDesc.g_ngroups.offset == L.ProblemDesc.g_u.offset + 16
    assert L.ProblemDesc.g_l1.offset == L.ProblemDesc.g_u.offset + 24 and L.ProblemDesc.g_lo.offset == L.ProblemDesc.g_u.offset + 32
    assert names[names.index("f_rows") + 1] == "f_classes" and names[names.index("f_classes") + 1] == "g_lambda"
    assert names[names.index("g_lambda_vec") - 1] == "g_hi_vec" and names[names.index("g_lambda_vec") + 1] == "c_A"
    assert names[-9:] == ["f_sp_nnz", "f_loss", "f_loss_delta", "f_w", "f_scale", "c_sp_rowptr", "c_sp_col", "c_sp_val", "c_sp_nnz"]
    assert L.BZ_G_CALLBACK == 8 and L.BZ_G_NORM_L21 == 9 and L.BZ_G_GROUP_LASSO == 10
    header = open(os.path.join(ROOT, "include", "bazinga_hip.h")).read()
    assert re.search(r"#define BZ_G_GROUP_LASSO\s+10\b", header)
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"const void\*\s+g_u;\s*const int64_t\*\s+g_group_ptr;\s*int64_t\s+g_ngroups;\s*double\s+g_l1;\s*double\s+g_lo, g_hi;", body)


def test_a_foreign_f_sends_all_four_kinds_to_callbacks(bz):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib

    class MyF:
        def gradient(self, dfx, x):
            dfx[...] = x
            return 0.5 * float(x @ x)
    g = bz.GroupLasso(0.5, [0, 2, 3, 8], l1=0.05)
    desc, keep = lower(MyF(), g, bz.IdentityFunction(), bz.FreeSet(), 8, 8, np.float64)
    assert (desc.f_kind, desc.g_kind, desc.c_kind, desc.D_kind) == (L.BZ_F_CALLBACK, L.BZ_G_CALLBACK, L.BZ_C_CALLBACK, L.BZ_D_CALLBACK)
    assert not desc.g_group_ptr and desc.g_ngroups == 0
    # ... where the numpy class is the prox the library calls back
    x = np.array([3.0, 4.0, 0.1, 0.1, 0, 0, 1, 0])
    z = (C.c_double * 8)()
    xb = (C.c_double * 8)(*x)
    v = desc.cb_g_prox(None, C.addressof(xb), 1.0, C.addressof(z), 8)
    want = np.empty(8)
    wv = g.prox(want, x, 1.0)
    assert np.array_equal(np.array(z), want) and v == wv and want[2] == 0 and want[0] != 0


def test_julia_shim_names_the_type():
    src = open(os.path.join(ROOT, "julia", "BazingaHIP.jl")).read()
    assert re.search(r"struct GroupLasso\b", src)
    assert re.search(r"ptr::Vector\{Int64\}", src) and re.search(r"Int64\[0; cumsum\(", src)
    assert re.search(r"lower_g!\(d, g::GroupLasso\{<:Real\}\) = \(d\.g_kind = 10; d\.g_group_ptr = pointer\(g\.ptr\); d\.g_ngroups = length\(g\.ptr\) - 1; "
                     r"d\.g_l1 = g\.l1; d\.g_lambda = g\.lambda\)", src)
    assert re.search(r"lower_g!\(d, g::GroupLasso\{<:AbstractVector\}\) = \(d\.g_kind = 10; .*d\.g_lambda_vec = pointer", src)
    m = re.search(r"mutable struct ProblemDesc\n(.*?)\nend", src, re.S)
    assert re.search(r"g_u::Ptr\{Cvoid\} = C_NULL\s+g_group_ptr::Ptr\{Cvoid\} = C_NULL; g_ngroups::Int64 = 0; g_l1::Float64 = 0", m.group(1))
