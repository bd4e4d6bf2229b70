"""The group Lasso over a group pointer on the device (BZ_G_GROUP_LASSO, k_fbstep_ragged of bz_group_ragged.h):
g(x) = l1 ||x||_1 + sum_j lambda_j ||x[ptr[j] : ptr[j+1]]||_2.  Creation and refusals through the raw ABI, one prox bit for bit
against the numpy class bz.GroupLasso (which is the specification) over the size patterns at which the lane map changes,
special values, thirty states against the oracle's PANOCplus with that class as g, a whole solve with dummy-coded groups,
lambda set along a path, and that the kind changes nothing else.  Tolerances and helpers are the sibling's
(tests/test_gpu_group_lasso.py)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.test_gpu_group_lasso import BASE, BLOCK, PSTRIDE, RTOL_SUM, group_counts, traces

pytestmark = pytest.mark.gpu

HOLD = 4                          # bz_group_ragged.h: RAGGED_HOLD, the trips of a group held in registers
MIX = [1, 2, 3, 5, 8, 13, 1, 40]


def lanes_of(sizes):
    """ragged_lanes of bz_group_ragged.h: the power of two >= the mean size, 64 at the most"""
    n, ng, L = int(np.sum(sizes)), len(sizes), 1
    while L < 64 and L * ng < n:
        L *= 2
    return L


def form_lanes(form, sizes):
    """(L, L1) of the profile's kernel name; LONG, the form with the second sweep, is launched exactly where a group exceeds
    the HOLD trips held in registers"""
    m = re.fullmatch(r"k_fbstep_ragged<L=(\d+),NT=([01]),L1=([01]),LONG=([01])>", form)
    assert m, form
    assert int(m.group(4)) == int(max(sizes) > HOLD * int(m.group(1))), form
    return int(m.group(1)), int(m.group(3))


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, sizes, lam=0.5, l1=0.0, f=None, c=None, D=None, ny=None, dtype=np.float64):
    """a good descriptor from lower(), then the raw fields"""
    from bazinga_jl_amd.oracles import lower
    n = int(np.sum(sizes))
    desc, keep = lower(f or bz.Zero(), bz.GroupLasso.from_sizes(0.5, sizes), c or bz.IdentityFunction(), D or bz.FreeSet(),
                       n, ny or n, dtype)
    desc.g_l1 = l1
    arr = None
    if np.ndim(lam) == 0:
        desc.g_lambda = lam
    else:
        arr = np.ascontiguousarray(lam, dtype)
        desc.g_lambda_vec = arr.ctypes.data
    return desc, [keep, arr]


def test_creation_validates_and_refuses_what_is_not_lowered(bz, ref):
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    sizes = [3, 1, 7, 2, 70, 5, 8]
    ng, n = len(sizes), sum(sizes)

    def create(desc, ctx=ctx, keep_it=False):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value and not keep_it:
            lib.bz_problem_destroy(h)
        return (rc, bool(h.value), msg) if not keep_it else h

    def refused(desc, code, *words, ctx=ctx):
        rc, made, msg = create(desc, ctx)
        assert rc == code and not made and "GroupLasso" in msg and all(w in msg for w in words), (rc, msg)

    desc, keep = raw_desc(bz, sizes)
    assert desc.g_kind == 10 and desc.g_ngroups == ng and create(desc)[:2] == (0, True)
    for good in ([1] * 24, [24], [23, 1], [1, 200, 1]):
        desc, keep = raw_desc(bz, good, lam=np.linspace(0.0, 1.0, len(good)), l1=0.25)
        assert create(desc)[:2] == (0, True)
    # the pointer rules
    for bad, word in (([1, 4, 11, 13, 83, 88, 96, 97], "[0]"), ([0, 3, 3, 11, 13, 83, 88, 96], "group 1"),
                      ([0, 4, 3, 11, 13, 83, 88, 96], "group 1"), ([0, 3, 4, 11, 13, 83, 88, 95], "must be n"),
                      ([0, 3, 4, 11, 13, 83, 88, 97], "must be n")):
        desc, keep = raw_desc(bz, sizes)
        p = np.array(bad, np.int64)
        keep.append(p)
        desc.g_group_ptr = p.ctypes.data
        refused(desc, L.BZ_ERR_ARG, "g_group_ptr", word)
    desc, keep = raw_desc(bz, sizes)
    desc.g_group_ptr = None
    refused(desc, L.BZ_ERR_ARG, "g_group_ptr", "null")
    for bad in (0, -1, n + 1):
        desc, keep = raw_desc(bz, sizes)
        desc.g_ngroups = bad
        refused(desc, L.BZ_ERR_ARG, "g_ngroups")
    # lambda and l1: finite and >= 0, a vector entry by entry
    for bad in (-0.5, np.inf, np.nan):
        desc, keep = raw_desc(bz, sizes, lam=bad)
        refused(desc, L.BZ_ERR_ARG, "g_lambda")
        desc, keep = raw_desc(bz, sizes, l1=bad)
        refused(desc, L.BZ_ERR_ARG, "g_l1")
        v = np.full(ng, 0.5)
        v[4] = bad
        desc, keep = raw_desc(bz, sizes, lam=v)
        refused(desc, L.BZ_ERR_ARG, "entry 4")
    # a pointer or a vector beside the wrong kind is an argument error; g_ngroups and g_l1 alone are ignored
    desc, keep = raw_desc(bz, sizes)
    desc.g_kind = L.BZ_G_NORM_L1
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "g_group_ptr" in msg and "GroupLasso alone" in msg
    desc.g_group_ptr = None
    assert desc.g_ngroups == ng and create(desc)[:2] == (0, True)
    desc, keep = raw_desc(bz, sizes, lam=np.full(ng, 0.5))
    desc.g_kind, desc.g_group_ptr = L.BZ_G_NORM_L1_NONNEG, None
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "NormL1 alone" in msg
    # the three refusals
    desc, keep = raw_desc(bz, sizes)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, sizes)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "one rank", ctx=ctx2)
    for field, kind in (("f_kind", L.BZ_F_CALLBACK), ("c_kind", L.BZ_C_CALLBACK), ("D_kind", L.BZ_D_CALLBACK)):
        desc, keep = raw_desc(bz, sizes)
        setattr(desc, field, kind)
        refused(desc, L.BZ_ERR_UNSUPPORTED, "callbacks")
    # the f, c and D of the kernel chain are taken
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, n))
    Ac = rng.standard_normal((3, n))
    sp = bz.SparseLeastSquares.from_dense(A, np.ones(6))
    for f in (bz.Zero(), bz.DiagQuadratic(np.ones(n), np.ones(n)), bz.LeastSquares(A, np.ones(6)), sp,
              bz.SparseLogistic.from_dense(A, np.array([1.0, -1, 1, -1, 1, 1]))):
        for D in (bz.ZeroSet(), bz.FreeSet(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)), bz.XorPairs()):
            desc, keep = raw_desc(bz, sizes, f=f, D=D)
            assert create(desc)[:2] == (0, True), (type(f).__name__, type(D).__name__)
    for c in (bz.DenseAffine(Ac, np.zeros(3)), bz.SparseAffine.from_dense(Ac, np.zeros(3))):
        desc, keep = raw_desc(bz, sizes, f=bz.DiagQuadratic(np.ones(n), np.ones(n)), c=c, D=bz.ZeroSet(), ny=3)
        assert create(desc)[:2] == (0, True)
    # bz_problem_set_g_lambda: a number for a number, a vector for a vector; a refused call changes nothing
    x = rng.standard_normal(n)

    def prox_of(h):
        z, gz = np.empty(n), C.c_double()
        assert lib.bz_eval_prox(h, x.ctypes.data, 0.7, z.ctypes.data, C.byref(gz)) == 0
        return z, gz.value

    def setter(h, lam, vec):
        rc = lib.bz_problem_set_g_lambda(h, lam, None if vec is None else vec.ctypes.data)
        return rc, (lib.bz_last_error().decode() if rc else "")

    want = np.empty(n)
    for l1 in (0.0, 0.2):
        desc, keep = raw_desc(bz, sizes, lam=0.5, l1=l1)
        h = create(desc, keep_it=True)
        before = prox_of(h)
        for bad in (-1.0, np.nan, np.inf):
            rc, msg = setter(h, bad, None)
            assert rc == L.BZ_ERR_ARG and "GroupLasso" in msg
        rc, msg = setter(h, 0.0, np.full(ng, 0.25))
        assert rc == L.BZ_ERR_ARG and "GroupLasso" in msg and "number" in msg
        after = prox_of(h)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
        assert setter(h, 0.9, None)[0] == 0
        wv = bz.GroupLasso.from_sizes(0.9, sizes, l1).prox(want, x, 0.7)
        got = prox_of(h)
        assert np.array_equal(got[0], want) and abs(got[1] - wv) <= 1e-12 * wv
        o = L.PanocOpts()
        lib.bz_panoc_default_opts(C.byref(o))
        ones, zeros = np.ones(n), np.zeros(n)
        assert lib.bz_problem_set_multipliers(h, ones.ctypes.data, zeros.ctypes.data) == 0
        assert lib.bz_panoc_begin(h, C.byref(o), x.ctypes.data) == 0
        assert setter(h, 0.3, None)[0] == L.BZ_ERR_STATE
        assert lib.bz_panoc_finish(h, None, None) == 0
        assert setter(h, 0.3, None)[0] == 0
        lib.bz_problem_destroy(h)
    v0 = np.linspace(0.0, 1.0, ng)
    desc, keep = raw_desc(bz, sizes, lam=v0, l1=0.2)
    h = create(desc, keep_it=True)
    before = prox_of(h)
    rc, msg = setter(h, 0.5, None)
    assert rc == L.BZ_ERR_ARG and "GroupLasso" in msg and "vector" in msg
    bad = v0.copy()
    bad[2] = -1.0
    rc, msg = setter(h, 0.0, bad)
    assert rc == L.BZ_ERR_ARG and "GroupLasso" in msg and "entry 2" in msg
    after = prox_of(h)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    v1 = v0[::-1].copy()
    assert setter(h, 0.0, v1)[0] == 0
    wv = bz.GroupLasso.from_sizes(v1, sizes, 0.2).prox(want, x, 0.7)
    got = prox_of(h)
    assert np.array_equal(got[0], want) and abs(got[1] - wv) <= 1e-12 * wv
    lib.bz_problem_destroy(h)
    # the Python layer raises before any device call
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.GroupLasso.from_sizes(0.5, sizes), bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64, slack=True)
    with pytest.raises(ValueError):
        bz.Problem(bz.Zero(), bz.GroupLasso.from_sizes(0.5, sizes), bz.IdentityFunction(), bz.FreeSet(), n + 1, n + 1, np.float64)


# ---- 2. one prox, bit for bit against the numpy class
def between(S, pairs):
    """a single group of S between groups of 1 and 2"""
    return [1, 2] * pairs + [S] + [2, 1] * pairs


def patterns():
    """(name, sizes, the lanes the solver must choose or None)"""
    out = [("ones", [1] * 1000, 1)]
    for K in (3, 8, 64):
        for ng in group_counts(K):
            if ng <= 1000:                                   # (the second grid trip is taken by the groups of 1 below)
                out.append((f"uniform{K}x{ng}", [K] * ng, None))
    out.append(("mix", MIX * 37, 16))
    for S in (63, 64, 65, 127, 128, 129, 1000, 4097):
        out.append((f"single{S}", between(S, 3), None))                # (L = 8 at 63 .. 64 at 4097: all sweep twice)
    # ... and among many small groups: few lanes, many accumulators in each
    out.append(("single65/L2", between(65, 1500), 2))
    out.append(("single1000/L2", between(1000, 1500), 2))
    out.append(("single4097/L4", between(4097, 1500), 4))
    # the register-held limit HOLD * L: just below, at and above, at L = 2, 8 and 64
    out.append(("hold/L2", [1] * 300 + [2 * HOLD - 1] + [1] * 40 + [2 * HOLD] + [1] * 77 + [2 * HOLD + 1] + [1] * 5, 2))
    out.append(("hold/L8", [8, 7] * 200 + [8 * HOLD - 1] + [8, 7] * 3 + [8 * HOLD] + [7] * 5 + [8 * HOLD + 1] + [8, 7] * 4, 8))
    out.append(("hold/L64", [60] * 9 + [64 * HOLD - 1] + [60] * 3 + [64 * HOLD] + [60] * 4 + [64 * HOLD + 1] + [60], 64))
    out.append(("whole", [5000], 64))
    # many groups above 128 elements, where the order of a group's sum shows (an ulp of the norm reaches z in about one
    # balanced group of six): on 64 lanes, and on 4 lanes with 16 accumulators each
    longs = [129, 191, 200, 255, 256, 257, 300, 500, 1000, 1025, 2049, 4097] * 3
    out.append(("order/L64", longs, 64))
    out.append(("order/L4", [g for S in longs for g in [1, 2] * 400 + [S]], 4))
    # group counts that leave a wave ragged: 64 / L - 1 and 64 / L + 1 groups, at L = 8 and at L = 4
    r8, r4 = [8, 3, 13, 5, 1, 9, 7], [3, 1, 5, 2, 4, 3, 1, 6, 2, 3, 4, 1, 5, 2, 3]
    out.append(("ragged7/L8", r8, 8))
    out.append(("ragged9/L8", r8 + [2, 10], 8))
    out.append(("ragged15/L4", r4, 4))
    out.append(("ragged17/L4", r4 + [4, 2], 4))
    # the first group count at which the grid-stride loop takes a second trip: PSTRIDE workgroups of BLOCK groups, and one more
    out.append(("second_trip", [1] * (PSTRIDE * BLOCK + 1), 1))
    return out


PATTERNS = patterns()


def planted(sizes, dtype, lam, gamma, l1, seed):
    """x with planted groups: one all zero and, with l1 == 0, one exactly at the threshold"""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    ng = len(sizes)
    x = rng.standard_normal(ptr[-1]).astype(dtype)
    lamv = np.asarray(lam, dtype) if np.ndim(lam) else np.full(ng, lam, dtype)
    where = {}
    if ng >= 4:
        jz, jt = rng.permutation(ng)[:2]
        x[ptr[jz]:ptr[jz + 1]] = 0
        where["zero"] = jz
        if l1 == 0:
            # y = (gl, 0, ...): sqrt(gl * gl) = gl exactly, so nrm <= gl holds with equality
            x[ptr[jt]:ptr[jt + 1]] = 0
            x[ptr[jt]] = dtype(gamma) * lamv[jt]
            where["threshold"] = jt
    return x, ptr, where


def balanced(sizes, dtype, lam, gamma, l1, seed):
    """x with every group's norm (behind the threshold) at 0.8 .. 2 times gamma * lambda_j: z = (1 - gl / nrm) u then cancels
    and shows the last bit of nrm — with N(0, 1) entries and gl << nrm a long group's z hides a wrong order of the sum.
    Groups with a factor below 1 go to zero; an unpenalised group keeps N(0, 1) entries."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    ng = len(sizes)
    v = rng.standard_normal(ptr[-1])
    gl = gamma * (np.asarray(lam, np.float64) if np.ndim(lam) else np.full(ng, lam))
    nrm = np.sqrt(np.add.reduceat(v * v, ptr[:-1]))
    r = np.where(gl > 0, rng.uniform(0.8, 2.0, ng) * gl / nrm, 1.0)
    u = v * np.repeat(r, sizes)
    return (u + np.sign(u) * (gamma * l1)).astype(dtype)


@pytest.mark.parametrize("l1", [0.0, 0.3], ids=["pure", "l1"])
@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_prox_bit_for_bit(bz, dtype, vector, l1):
    """z equals the numpy class bit for bit and g(z) within RTOL_SUM, pattern by pattern, on N(0, 1) entries with planted
    groups and on entries balanced against the threshold; where the sizes are equal and l1 == 0, z also equals the device
    output of a NormL21 problem"""
    gamma = 0.37
    for name, sizes, lanes in PATTERNS:
        ng, n = len(sizes), int(np.sum(sizes))
        if vector:
            lam = 0.6 * np.random.default_rng(ng).uniform(0.2, 1.0, ng)
            lam[::7] = 0.0
        else:
            lam = 0.8
        gnum = bz.GroupLasso.from_sizes(lam, sizes, l1)
        x, ptr, where = planted(sizes, dtype, lam, gamma, l1, 7 * ng + n)
        prob = bz.Problem(bz.Zero(), gnum, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
        z, gz = prob.eval_prox(x, gamma)
        L_dev, l1_dev = form_lanes(prob.profile2()["fb_step"]["form"], sizes)
        assert L_dev == lanes_of(sizes) and (lanes is None or L_dev == lanes) and l1_dev == int(l1 > 0), (name, L_dev)
        want = np.empty_like(x)
        wv = gnum.prox(want, x, dtype(gamma))
        bad = np.flatnonzero(z != want)
        assert bad.size == 0, (name, bad[:8], np.searchsorted(ptr, bad[:8], side="right") - 1)
        assert np.array_equal(np.signbit(z), np.signbit(want)), name
        for kind, j in where.items():
            assert np.all(z[ptr[j]:ptr[j + 1]] == 0), (name, kind)
        assert np.isfinite(gz) and abs(gz - float(wv)) <= RTOL_SUM[dtype] * max(1.0, abs(float(wv))), (name, gz, wv)
        xb = balanced(sizes, dtype, lam, gamma, l1, 3 * ng + n)
        zb, gzb = prob.eval_prox(xb, gamma)
        wvb = gnum.prox(want, xb, dtype(gamma))
        bad = np.flatnonzero(zb != want)
        assert bad.size == 0, (name, "balanced", bad[:8], np.searchsorted(ptr, bad[:8], side="right") - 1)
        assert np.array_equal(np.signbit(zb), np.signbit(want)), name
        assert ng < 20 or (np.any(zb != 0) and np.any(zb == 0)), name
        assert np.isfinite(gzb) and abs(gzb - float(wvb)) <= RTOL_SUM[dtype] * max(1.0, abs(float(wvb))), (name, gzb, wvb)
        prob.close()
        if name.startswith("uniform") and l1 == 0:
            K = sizes[0]
            p9 = bz.Problem(bz.Zero(), bz.NormL21(lam, K), bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
            z9, gz9 = p9.eval_prox(x, gamma)
            p9.close()
            assert np.array_equal(z9.view(np.uint8), z.view(np.uint8)), name
            assert abs(gz9 - gz) <= RTOL_SUM[dtype] * max(1.0, abs(gz)), name


# ---- 3. special values
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_special_values(bz, dtype):
    T = dtype
    gamma = 0.5
    sizes = [4, 70, 3, 300, 5, 1, 2]                         # (L = 64: the group of 300 sweeps twice)
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    n = int(ptr[-1])
    rng = np.random.default_rng(3)
    lam = np.array([0.5, 0.25, 1.0, 0.3, 0.0, 0.7, 0.2])
    base = rng.standard_normal(n).astype(T)
    base[ptr[1]:ptr[2]] = 0                                  # an all-zero group of 70
    base[ptr[2]:ptr[3]] = [0, T(gamma) * T(lam[2]), 0]       # nrm exactly gamma * lambda_j
    base[ptr[4]:ptr[5]] = [1.5, -0.0, 0.0, -0.0, -2.0]       # lambda_j = 0: y bit for bit with l1 == 0
    for l1 in (0.0, 0.5):
        g = bz.GroupLasso(lam, ptr, l1)
        prob = bz.Problem(bz.Zero(), g, bz.IdentityFunction(), bz.FreeSet(), n, n, T)
        x = base.copy()
        if l1 > 0:
            t = T(gamma) * T(l1)                             # 0.25: the ties |y| = gamma * l1, and both zeros
            x[ptr[3]:ptr[3] + 4] = [t, -t, 0.0, -0.0]
            x[ptr[2]:ptr[3]] = [0, T(gamma) * T(lam[2]) + t, 0]          # u = (0.5 + 0.25) - 0.25 = gamma * lambda_j exactly
        z, gz = prob.eval_prox(x, gamma)
        want = np.empty_like(x)
        wv = g.prox(want, x, T(gamma))
        assert np.array_equal(z.view(np.uint8), want.view(np.uint8))
        assert np.all(z[ptr[1]:ptr[3]] == 0) and not np.any(np.signbit(z[ptr[1]:ptr[3]]))
        assert abs(gz - float(wv)) <= RTOL_SUM[T] * max(1.0, abs(float(wv)))
        if l1 == 0:
            assert np.array_equal(z[ptr[4]:ptr[5]].view(np.uint8), x[ptr[4]:ptr[5]].view(np.uint8))      # (-0 stays -0)
        else:
            assert np.all(z[ptr[3]:ptr[3] + 4] == 0) and not np.any(np.signbit(z[ptr[3]:ptr[3] + 4]))
            assert np.any(z[ptr[3] + 4:ptr[4]] != 0)
        # the zero group adds nothing to g: the value without it is the same
        keep = np.r_[0:ptr[1], ptr[2]:n]
        g2 = bz.GroupLasso.from_sizes(np.delete(lam, 1), np.delete(sizes, 1), l1)
        assert g2.prox(np.empty(keep.size, T), x[keep], T(gamma)) == wv
        # a NaN in one group makes that group NaN and leaves every other group's bits as they were
        for j in (3, 0):
            xn = x.copy()
            xn[ptr[j + 1] - 2] = np.nan
            zn, gn = prob.eval_prox(xn, gamma)
            inside = np.zeros(n, bool)
            inside[ptr[j]:ptr[j + 1]] = True
            assert np.all(np.isnan(zn[inside])) and np.isnan(gn)
            assert np.array_equal(zn[~inside].view(np.uint8), z[~inside].view(np.uint8))
        prob.close()


# ---- 4. the step with a gradient, and thirty states against the oracle
STATE_SIZES = {"diag": MIX * 12 + [100, 24], "sparse_ls": [1, 2, 3, 5, 8, 13, 1, 70, 25]}


def state_problem(bz, ref, name, dtype, l1):
    sizes = STATE_SIZES[name]
    n = sum(sizes)
    if name == "diag":
        d = bz.synth.l1_quadratic(n, dtype=dtype)
        lam = 12.0 * np.linspace(0.5, 1.5, len(sizes))
        lam[0] = 0.0
        g = bz.GroupLasso.from_sizes(lam, sizes, 4.0 * l1)
        box = (bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])), ref.ClosedSet(ref.IndBox(dtype(d["lo"]), dtype(d["hi"]))))
        return n, (bz.DiagQuadratic(d["q"], d["b"]), g, bz.IdentityFunction(), box[0]), \
            (ref.DiagQuadratic(d["q"], d["b"]), g, ref.IdentityFunction(), box[1])
    m = 60
    d = bz.synth.sparse_lasso(m, n, 5, dtype)
    f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], n)
    g = bz.GroupLasso.from_sizes(0.1, sizes, 0.1 * l1)
    box = (bz.ClosedSet(bz.IndBox(-1.0, 1.0)), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1))))
    return n, (f, g, bz.IdentityFunction(), box[0]), (ref.LeastSquares(f.toarray(), d["b"]), g, ref.IdentityFunction(), box[1])


def test_the_step_with_a_gradient(bz):
    """z = prox(x0 - gamma grad), res = x0 - z and the three sums of the first state, with an explicit step size"""
    for dtype in (np.float64, np.float32):
        for l1 in (0.0, 0.3):
            sizes = STATE_SIZES["diag"]
            n, gamma = sum(sizes), 0.37
            rng = np.random.default_rng(11)
            x0, g = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
            gnum = bz.GroupLasso.from_sizes(0.8, sizes, l1)
            # f = DiagQuadratic(0, -g): grad f(x) = g exactly; with c = Identity, D = Free and y = 0 it is the gradient the step sees
            prob = bz.Problem(bz.DiagQuadratic(np.zeros(n, dtype), -g), gnum, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
            prob.set_multipliers(np.ones(n, dtype), np.zeros(n, dtype))
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, gamma=gamma, adaptive=False).c_opts(), x0)
            sc = prob.panoc_scalars()
            zd, rd, gd = prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_vector("grad_x")
            prob.panoc_finish()
            prob.close()
            assert np.array_equal(gd, g) and sc["gamma"] == float(dtype(gamma)) and sc["fused"] == 0
            want = np.empty_like(x0)
            wv = gnum.prox(want, x0 - dtype(gamma) * g, dtype(gamma))
            res = x0 - want
            assert np.array_equal(zd, want) and np.array_equal(rd, res)
            tol = RTOL_SUM[dtype]
            assert abs(sc["g_z"] - float(wv)) <= tol * max(1.0, abs(float(wv)))
            dot = float(np.sum((g * res).astype(np.float64)))
            ss = float(np.sum((res * res).astype(np.float64)))
            scale = float(np.sum(np.abs((g * res).astype(np.float64))))
            assert abs(sc["dot_grad_res"] - dot) <= tol * max(1.0, scale)
            assert abs(sc["ss_res"] - ss) <= tol * max(1.0, ss)


STATES = [("diag", np.float64, 0.0), ("diag", np.float64, 0.3), ("diag", np.float32, 0.3), ("sparse_ls", np.float64, 0.0),
          ("sparse_ls", np.float64, 0.3), ("sparse_ls", np.float32, 0.0)]


@pytest.mark.parametrize("name,dtype,l1", STATES, ids=[f"{s[0]}-{'f64' if s[1] is np.float64 else 'f32'}-l1={s[2]}" for s in STATES])
def test_iterates_follow_the_oracle(bz, ref, name, dtype, l1):
    """30 states of the oracle's PANOCplus with the numpy class as g, under the sibling's rule: x and z inside
    max(base, 100 * sens), gamma equal to 1e-12 / 1e-5 relative, g(z) to the same bound"""
    n, dev, orc = state_problem(bz, ref, name, dtype, l1)
    mu, y = np.full(n, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(n)).astype(dtype)
    x0 = np.zeros(n, dtype)
    prob, rows = traces(bz, ref, dev, orc, n, n, mu, y, x0, 30, dtype, None)
    pr = prob.profile2()
    stats = prob.panoc_stats()
    prob.close()
    base = BASE[dtype]
    for k, ex, ez, g_d, g_r, gz_d, gz_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} g_z {gz_d:.12g} / {gz_r:.12g} sens={sens:.3e}")
    for k, ex, ez, g_d, g_r, gz_d, gz_r, fused, sens in rows:
        assert np.isfinite(g_r) and abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
        assert abs(gz_d - gz_r) <= max(base, 100 * sens) * max(1.0, abs(gz_r)), (k, gz_d, gz_r)
        assert fused == 0
    L_dev, l1_dev = form_lanes(pr["fb_step"]["form"], STATE_SIZES[name])
    assert L_dev == lanes_of(STATE_SIZES[name]) and l1_dev == int(l1 > 0)
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0 and stats.n_fused_iters == 0
    assert len({r[1] for r in rows}) > 1 or rows[-1][1] == 0.0
    assert len({r[5] for r in rows}) > 1                     # (the penalty is at work)


# ---- 5. a whole alps solve with dummy-coded groups
def dummy_coded(seed=0):
    """m = 240 rows of an intercept column and 14 factors of 2 .. 9 levels, one indicator column per level; the response
    depends on the intercept and on five of the factors"""
    rng = np.random.default_rng(seed)
    levels = [2, 9, 3, 5, 7, 4, 8, 6, 2, 3, 9, 5, 4, 6]
    m = 240
    sizes = [1] + levels
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    A = np.zeros((m, ptr[-1]))
    A[:, 0] = 1.0
    b = np.full(m, 1.5)
    for f, nl in enumerate(levels):
        lv = rng.integers(0, nl, m)
        A[np.arange(m), ptr[f + 1] + lv] = 1.0
        if f in (1, 3, 6, 9, 11):
            eff = rng.standard_normal(nl)
            eff[rng.permutation(nl)[:nl // 2]] *= 0.02          # (levels that hardly matter: the l1 mix drops them)
            b += (eff - eff.mean())[lv]
    b += 0.1 * rng.standard_normal(m)
    return A / np.sqrt(m), b / np.sqrt(m), sizes, ptr


@pytest.mark.parametrize("l1", [0.0, 0.01], ids=["pure", "l1"])
def test_whole_solve_with_dummy_coded_groups(bz, ref, l1):
    """device and oracle agree on the status and on the set of all-zero groups; at least a third of the factors are dropped
    and at least a quarter kept; the unpenalised intercept (a group of one, lambda = 0) is non-zero; with l1 > 0 zeros sit
    inside active groups in both"""
    A, b, sizes, ptr = dummy_coded()
    n, ng = int(ptr[-1]), len(sizes)
    lam = 0.03 * np.sqrt(np.array(sizes, float))
    lam[0] = 0.0
    g = bz.GroupLasso(lam, ptr, l1)
    f = bz.SparseLeastSquares.from_dense(A, b)
    box = (bz.ClosedSet(bz.IndBox(-50.0, 50.0)), ref.ClosedSet(ref.IndBox(-50.0, 50.0)))
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(ref.LeastSquares(A, b), g, ref.IdentityFunction(), box[1], np.zeros(n), np.zeros(n), subsolver=subr, subsolver_maxit=100000)
    a = bz.alps(f, g, bz.IdentityFunction(), box[0], np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000)

    def zero_groups(x):
        return np.array([np.all(x[ptr[j]:ptr[j + 1]] == 0) for j in range(ng)])
    zero_o, zero_a = zero_groups(o[0]), zero_groups(a[0])
    print(f"status {a[5]} / {o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} zero groups {zero_a.sum()}/{zero_o.sum()} "
          f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert o[5] == "first_order" and zero_o.sum() >= (ng - 1) // 3 and (~zero_o).sum() >= (ng - 1) // 4, (o[5], zero_o.sum())
    assert a[5] == o[5]
    assert np.array_equal(zero_a, zero_o)
    for x in (a[0], o[0]):
        assert x[0] != 0
        inner = sum(int(np.count_nonzero(x[ptr[j]:ptr[j + 1]] == 0)) for j in range(1, ng) if np.any(x[ptr[j]:ptr[j + 1]] != 0))
        assert (inner > 0) == (l1 > 0), inner


# ---- 6. set_g_lambda along a path
@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
def test_lambda_path_on_a_live_problem(bz, vector):
    """three values on one problem: each solve equals a fresh problem's bit for bit"""
    A, b, sizes, ptr = dummy_coded(1)
    n = int(ptr[-1])
    f = bz.SparseLeastSquares.from_dense(A, b)
    rest = (bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-50.0, 50.0)))
    base = 0.03 * np.sqrt(np.array(sizes, float))
    base[0] = 0.0
    path = [s * base if vector else s * 0.06 for s in (2.0, 1.0, 0.5)]
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    live = bz.Problem(f, bz.GroupLasso(path[0], ptr, 0.005), *rest, n, n, np.float64)
    sols = []
    for i, lam in enumerate(path):
        if i:
            live.set_g_lambda(lam)
        g = bz.GroupLasso(lam, ptr, 0.005)
        got = bz.alps(f, g, *rest, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, problem=live)
        fresh = bz.alps(f, g, *rest, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, resident=True)
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]) and got[2:4] == fresh[2:4] and got[5] == fresh[5]
        sols.append(got[0])
    with pytest.raises(bz.BazingaHipError):
        live.set_g_lambda(base if not vector else 0.5)                 # number <-> vector stays a creation-time decision
    live.close()
    assert not np.array_equal(sols[0], sols[1]) and not np.array_equal(sols[1], sols[2])


# ---- 7. nothing else moves
def test_norm_l21_and_norm_l1_keep_their_kernels_and_bits(bz, ref):
    n, K = 20011 - 1, 5
    d = bz.synth.l1_quadratic(n)
    rest = (bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
    sub = bz.PANOCplus(tol=1e-8, maxit=60)
    out = {}
    for name, g in (("group", bz.NormL21(d["lam"], K)), ("ragged", bz.GroupLasso.from_sizes(d["lam"], [K] * (n // K))),
                    ("l1", bz.NormL1(d["lam"]))):
        prob = bz.Problem(bz.DiagQuadratic(d["q"], d["b"]), g, *rest, n, n, np.float64)
        prob.set_multipliers(np.full(n, 0.1), np.zeros(n))
        x, st = prob.panoc_solve(sub.c_opts(), np.zeros(n))
        out[name] = (int(st.n_fused_iters), int(st.iters), prob.profile2(), x)
        prob.close()
    fused, iters, pr, x9 = out["group"]
    assert fused == 0 and iters > 3 and pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0
    assert pr["fb_step"]["form"] == "k_fbstep_group<KP=8,NT=0>"
    # (the bits NormL21 had: the class is its specification, and the new kind on equal sizes reproduces the whole solve)
    fused, iters10, pr, x10 = out["ragged"]
    assert fused == 0 and pr["fb_step"]["form"] == "k_fbstep_ragged<L=8,NT=0,L1=0,LONG=0>"
    assert iters10 == iters and np.array_equal(x9.view(np.uint8), x10.view(np.uint8))
    z9 = np.empty(n)
    xr = np.random.default_rng(1).standard_normal(n)
    prob = bz.Problem(bz.Zero(), bz.NormL21(0.4, K), bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64)
    z, gz = prob.eval_prox(xr, 0.37)
    prob.close()
    bz.NormL21(0.4, K).prox(z9, xr, 0.37)
    assert np.array_equal(z.view(np.uint8), z9.view(np.uint8))
    fused, iters, pr, x1 = out["l1"]
    assert fused > 0 and pr["k_fused_iterates"]["launches"] + pr["k_fused_sep"]["launches"] > 0
    # ... and NormL1's step has the bits of the reference's soft threshold (tests/test_gpu_parity.py::test_prox_bit_exact's check)
    prob = bz.Problem(bz.Zero(), bz.NormL1(0.4), bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64)
    z, gz = prob.eval_prox(xr, 0.37)
    prob.close()
    z1 = np.empty(n)
    v1 = ref.NormL1(0.4).prox(z1, xr, 0.37)
    assert np.array_equal(z, z1) and abs(gz - v1) <= 1e-13 * max(1.0, abs(v1))
