"""The group Lasso g on the device (BZ_G_NORM_L21, k_fbstep_group of bz_group.h): g(x) = sum_j lambda_j ||x[jK : (j+1)K]||_2.
Creation and refusals through the raw ABI, one prox bit for bit against the numpy class bz.NormL21 (which is the
specification: the reference package has no such type) over every group width and the group counts at which the lane map
changes, thirty states against the oracle's PANOCplus with that class as g, a whole grouped multinomial solve, lambda set
along a path, and that the kind changes nothing else."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import LongDoubleReducer, _err
from tests.test_gpu_sparse import CsrOracle
from tests.test_gpu_sparse_glm import what_of
from tests.test_gpu_sparse_multinomial import MultinomialOracle

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 33, 64]
BLOCK, PSTRIDE = 256, 2048        # bz_kernels.h: threads of a workgroup, the grid cap (group_grid of bz_group.h)
BASE = {np.float64: 1e-9, np.float32: 5e-5}        # the state comparison of tests/test_gpu_sparse_multinomial.py
RTOL_SUM = {np.float64: 1e-12, np.float32: 1e-5}   # reduced scalars, as the sibling tests compare gamma and the values


def kp_of(K):
    kp = 1
    while kp < K:
        kp *= 2
    return kp


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, n, K, lam=0.5, f=None, c=None, D=None, ny=None, dtype=np.float64):
    """a good descriptor from lower() (the group size 1 divides every n), then the raw fields"""
    from bazinga_jl_amd.oracles import lower
    desc, keep = lower(f or bz.Zero(), bz.NormL21(0.5, 1), c or bz.IdentityFunction(), D or bz.FreeSet(),
                       n, ny or n, dtype)
    desc.g_group = K
    arr = None
    if np.ndim(lam) == 0:
        desc.g_lambda = lam
    else:
        arr = np.ascontiguousarray(lam, dtype)
        desc.g_lambda_vec = arr.ctypes.data
    return desc, (keep, arr)


def test_creation_validates_and_refuses_what_is_not_lowered(bz, ref):
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    n, K = 24, 4

    def create(desc, ctx=ctx, keep_it=False):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value and not keep_it:
            lib.bz_problem_destroy(h)
        return (rc, bool(h.value), msg) if not keep_it else h

    def refused(desc, code, *words, ctx=ctx):
        rc, made, msg = create(desc, ctx)
        assert rc == code and not made and "NormL21" in msg and all(w in msg for w in words), (rc, msg)

    desc, keep = raw_desc(bz, n, K)
    assert desc.g_kind == 9 and desc.g_group == K and create(desc)[:2] == (0, True)
    for good in (1, 2, 3, 24):
        desc, keep = raw_desc(bz, n, good, lam=np.linspace(0.0, 1.0, n // good))
        assert create(desc)[:2] == (0, True)
    desc, keep = raw_desc(bz, 128, 64)
    assert create(desc)[:2] == (0, True)
    # g_group in 1 .. 64, n % g_group == 0
    for bad in (0, -1, 65, 128):
        desc, keep = raw_desc(bz, 128, bad)
        refused(desc, L.BZ_ERR_ARG, "g_group")
    desc, keep = raw_desc(bz, n, 5)
    refused(desc, L.BZ_ERR_ARG, "multiple")
    # lambda: finite and >= 0, a vector entry by entry
    for bad in (-0.5, np.inf, np.nan):
        desc, keep = raw_desc(bz, n, K, lam=bad)
        refused(desc, L.BZ_ERR_ARG, "g_lambda")
        v = np.full(n // K, 0.5)
        v[4] = bad
        desc, keep = raw_desc(bz, n, K, lam=v)
        refused(desc, L.BZ_ERR_ARG, "entry 4")
    # a vector beside any other kind but NormL1 is still an argument error
    desc, keep = raw_desc(bz, n, K, lam=np.full(n // K, 0.5))
    desc.g_kind = L.BZ_G_NORM_L1_NONNEG
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "NormL1 alone" in msg
    # the three refusals
    desc, keep = raw_desc(bz, n, K)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, n, K)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "one rank", ctx=ctx2)
    for field, kind in (("f_kind", L.BZ_F_CALLBACK), ("c_kind", L.BZ_C_CALLBACK), ("D_kind", L.BZ_D_CALLBACK)):
        desc, keep = raw_desc(bz, n, K)
        setattr(desc, field, kind)
        refused(desc, L.BZ_ERR_UNSUPPORTED, "callbacks")
    # every f, c and D of the kernel chain is taken
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, n))
    sp = bz.SparseLeastSquares.from_dense(A, np.ones(6))
    lab = np.array([0.0, 1, 2, 3, 0, 1])
    spA = bz.SparseLeastSquares.from_dense(A[:, :n // K], np.ones(6))
    fs = [bz.Zero(), bz.DiagQuadratic(np.ones(n), np.ones(n)), bz.Stencil5ptQuadratic(4, 6, np.ones(n)), bz.LeastSquares(A, np.ones(6)),
          bz.Quadratic(np.eye(n), np.ones(n)), bz.SparseQuadratic.from_dense(np.eye(n), np.ones(n)), sp,
          bz.SparseLogistic.from_dense(A, np.where(lab > 1, 1.0, -1.0)), bz.SparseGLM.from_dense(A, np.ones(6), "huber", delta=1.0),
          bz.SparseMultinomial(spA.indptr, spA.indices, spA.data, lab, n // K, K)]
    for f in fs:
        for D in (bz.ZeroSet(), bz.FreeSet(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)), bz.XorPairs()):
            if isinstance(f, bz.Stencil5ptQuadratic) and isinstance(D, bz.PairwiseSet):
                continue
            desc, keep = raw_desc(bz, n, K, f=f, D=D)
            assert create(desc)[:2] == (0, True), (type(f).__name__, type(D).__name__)
    Ac = rng.standard_normal((3, n))
    for f in (bz.Zero(), bz.DiagQuadratic(np.ones(n), np.ones(n)), bz.LeastSquares(A, np.ones(6))):
        desc, keep = raw_desc(bz, n, K, f=f, c=bz.DenseAffine(Ac, np.zeros(3)), D=bz.ZeroSet(), ny=3)
        assert create(desc)[:2] == (0, True)
    for f in (bz.Zero(), bz.DiagQuadratic(np.ones(n), np.ones(n)), sp):
        desc, keep = raw_desc(bz, n, K, f=f, c=bz.SparseAffine.from_dense(Ac, np.zeros(3)), D=bz.ZeroSet(), ny=3)
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

    desc, keep = raw_desc(bz, n, K, lam=0.5)
    h = create(desc, keep_it=True)
    before = prox_of(h)
    for bad in (-1.0, np.nan, np.inf):
        rc, msg = setter(h, bad, None)
        assert rc == L.BZ_ERR_ARG and "NormL21" in msg
    rc, msg = setter(h, 0.0, np.full(n // K, 0.25))
    assert rc == L.BZ_ERR_ARG and "NormL21" in msg and "number" in msg
    after = prox_of(h)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert setter(h, 0.9, None)[0] == 0
    want = np.empty(n)
    wv = bz.NormL21(0.9, K).prox(want, x, 0.7)
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
    v0 = np.linspace(0.0, 1.0, n // K)
    desc, keep = raw_desc(bz, n, K, lam=v0)
    h = create(desc, keep_it=True)
    before = prox_of(h)
    rc, msg = setter(h, 0.5, None)
    assert rc == L.BZ_ERR_ARG and "NormL21" in msg and "vector" in msg
    bad = v0.copy()
    bad[2] = -1.0
    rc, msg = setter(h, 0.0, bad)
    assert rc == L.BZ_ERR_ARG and "NormL21" in msg and "entry 2" in msg
    after = prox_of(h)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    v1 = v0[::-1].copy()
    assert setter(h, 0.0, v1)[0] == 0
    wv = bz.NormL21(v1, K).prox(want, x, 0.7)
    got = prox_of(h)
    assert np.array_equal(got[0], want) and abs(got[1] - wv) <= 1e-12 * wv
    lib.bz_problem_destroy(h)
    # the messages of the other kinds are what they were
    desc, keep = raw_desc(bz, n, K)
    desc.g_kind = L.BZ_G_IND_BOX
    h = create(desc, keep_it=True)
    rc, msg = setter(h, 0.5, None)
    assert rc == L.BZ_ERR_ARG and "NormL1, NormL1Nonneg, NormL1Box or NormL0Box" in msg
    lib.bz_problem_destroy(h)
    # the Python layer raises before any device call
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.NormL21(0.5, K), bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64, slack=True)
    with pytest.raises(ValueError):
        bz.Problem(bz.Zero(), bz.NormL21(0.5, 5), bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64)


# ---- 2. one prox, bit for bit against the numpy class
def group_counts(K):
    """a single group; a ragged wave (64 / KP - 1 and 64 / KP + 1 groups); 1000 groups: several workgroups; and, at KP = 64, the
    first count at which the grid-stride loop takes a second trip: PSTRIDE workgroups of BLOCK / KP groups each, and one more"""
    kp = kp_of(K)
    counts = {1, 64 // kp + 1, 1000}
    if 64 // kp - 1 >= 1:
        counts.add(64 // kp - 1)
    if kp == 64:
        counts.add(PSTRIDE * (BLOCK // kp) + 1)
    return sorted(counts)


def planted(ng, K, dtype, lam, gamma, with_g, seed):
    """x (and the gradient) with planted groups: zero, exactly at the threshold, NaN in the last element, +inf, -inf"""
    rng = np.random.default_rng(seed)
    n = ng * K
    x = rng.standard_normal(n).astype(dtype)
    g = rng.standard_normal(n).astype(dtype) if with_g else None
    lamv = np.asarray(lam, dtype) if np.ndim(lam) else np.full(ng, lam, dtype)
    slots = rng.permutation(ng)[:min(ng, 5)]
    kinds = ["zero", "threshold", "nan", "+inf", "-inf"][:len(slots)] if ng >= 5 else ["threshold"][:len(slots)]
    for j, kind in zip(slots, kinds):
        s = slice(j * K, (j + 1) * K)
        if kind == "zero":
            x[s] = 0
            if g is not None:
                g[s] = 0
        elif kind == "threshold":
            # y = (gl, 0, ...): sqrt(gl * gl) = gl exactly, so nrm <= gl holds with equality (lambda_j = 0: the zero group)
            gl = dtype(gamma) * lamv[j]
            x[s] = 0
            x[j * K] = gl
            if g is not None:
                g[s] = 0
        elif kind == "nan":
            x[(j + 1) * K - 1] = np.nan
        else:
            x[j * K + K // 2] = np.inf if kind == "+inf" else -np.inf
    return x, g, dict(zip(kinds, slots))


@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_prox_bit_for_bit(bz, dtype, K, vector):
    """z (and res) equal the numpy class bit for bit; the three sums against numpy sums of the same per-element terms"""
    L = bz._lib
    lib = L.load()
    gamma = 0.37
    for ng in group_counts(K):
        n = ng * K
        if vector:
            lam = 0.6 * np.random.default_rng(ng).uniform(0.2, 1.0, ng)
            lam[::7] = 0.0
        else:
            lam = 0.8
        gnum = bz.NormL21(lam, K)
        # f = DiagQuadratic(0, -g): grad f(x) = 0 x - (-g) = g exactly, and with c = Identity, D = Free and y = 0 the penalty's
        # part of grad L is 0: the vector g below IS the gradient the step sees (asserted)
        xg, g, whereg = planted(ng, K, dtype, lam, gamma, True, 11 * ng + K)
        xg = np.where(np.isfinite(xg), xg, dtype(0.25))
        prob = bz.Problem(bz.DiagQuadratic(np.zeros(n, dtype), -g), gnum, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
        # (a) the pure prox, res null: bz_eval_prox
        x, _, where = planted(ng, K, dtype, lam, gamma, False, 7 * ng + K)
        z, gz = prob.eval_prox(x, gamma)
        want = np.empty_like(x)
        with np.errstate(all="ignore"):
            wv = gnum.prox(want, x, dtype(gamma))
        assert np.array_equal(z, want, equal_nan=True), (ng, np.flatnonzero(~((z == want) | (np.isnan(z) & np.isnan(want))))[:8])
        assert np.array_equal(np.signbit(z), np.signbit(want)) or np.any(np.isnan(want))
        if "nan" in where:
            j = where["nan"]
            assert np.all(np.isnan(z[j * K:(j + 1) * K])) and np.isnan(z).sum() == K and np.isnan(gz)
            for kind in ("+inf", "-inf"):
                s = slice(where[kind] * K, (where[kind] + 1) * K)
                assert np.array_equal(z[s], x[s])
            assert np.all(z[where["zero"] * K:(where["zero"] + 1) * K] == 0)
        assert np.all(z[where["threshold"] * K:(where["threshold"] + 1) * K] == 0)
        # ... and its g value on a finite input
        xf = np.where(np.isfinite(x), x, dtype(0.25))
        z, gz = prob.eval_prox(xf, gamma)
        wv = gnum.prox(want, xf, dtype(gamma))
        assert np.array_equal(z, want) and np.isfinite(gz) and abs(gz - float(wv)) <= RTOL_SUM[dtype] * max(1.0, abs(float(wv))), (ng, gz, wv)
        # (b) with a gradient, res kept: the first state of a solve with an explicit step size (z = prox(x0 - gamma grad), res = x0 - z)
        prob.set_multipliers(np.ones(n, dtype), np.zeros(n, dtype))
        o = bz.PANOCplus(tol=0.0, maxit=10 ** 9, gamma=gamma, adaptive=False).c_opts()
        prob.panoc_begin(o, xg)
        sc = prob.panoc_scalars()
        zd, rd, gd = prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_vector("grad_x")
        prob.panoc_finish()
        assert np.array_equal(gd, g) and sc["gamma"] == float(dtype(gamma)) and sc["fused"] == 0
        y = xg - dtype(gamma) * g
        wv = gnum.prox(want, y, dtype(gamma))
        res = xg - want
        assert np.array_equal(zd, want) and np.array_equal(rd, res)
        for kind in ("zero", "threshold"):
            if kind in whereg:
                assert np.all(zd[whereg[kind] * K:(whereg[kind] + 1) * K] == 0)
        tol = RTOL_SUM[dtype]
        assert abs(sc["g_z"] - float(wv)) <= tol * max(1.0, abs(float(wv)))
        dot = float(np.sum((g * res).astype(np.float64)))
        ss = float(np.sum((res * res).astype(np.float64)))
        scale = float(np.sum(np.abs((g * res).astype(np.float64))))
        assert abs(sc["dot_grad_res"] - dot) <= tol * max(1.0, scale), (ng, sc["dot_grad_res"], dot)
        assert abs(sc["ss_res"] - ss) <= tol * max(1.0, ss), (ng, sc["ss_res"], ss)
        prob.close()


# ---- 3. thirty states against the oracle
def state_problem(bz, ref, name, dtype):
    """(n, ny, device oracles, reference oracles, the explicit first step size or None)"""
    if name.startswith("multinomial"):
        K = int(name.split("-")[1][1:])
        boxed = name.endswith("box")
        m, nf = 60, 12
        n = nf * K
        d = bz.synth.sparse_multinomial(m, nf, K, 5, dtype)
        f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], nf, K)
        fo = MultinomialOracle(f.toarray(), d["labels"], K, what_of(None, 1.0, dtype))
        lam = np.full(nf, 0.5 if K == 3 else 1.0)
        lam[0] = 0.0
        # D = Free: the step-size probe x0 + 1 leaves the softmax and the (flat) penalty unchanged — the estimate would be 0 — so
        # the first step size is given; with the box(-5, 0.5) the probe leaves the box and the estimate is the penalty's
        Dd, Dr = (bz.ClosedSet(bz.IndBox(-5.0, 0.5)), ref.ClosedSet(ref.IndBox(dtype(-5), dtype(0.5)))) if boxed else (bz.FreeSet(), ref.FreeSet())
        return n, n, (f, bz.NormL21(lam, K), bz.IdentityFunction(), Dd), (fo, bz.NormL21(lam, K), ref.IdentityFunction(), Dr), None if boxed else 0.1
    if name == "sparse_ls":
        m, n, K = 60, 128, 4
        d = bz.synth.sparse_lasso(m, n, 5, dtype)
        f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], n)
        box = (bz.ClosedSet(bz.IndBox(-1.0, 1.0)), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1))))
        return n, n, (f, bz.NormL21(0.1, K), bz.IdentityFunction(), box[0]), (ref.LeastSquares(f.toarray(), d["b"]), bz.NormL21(0.1, K), ref.IdentityFunction(), box[1]), None
    if name == "diag":
        n, K = 1000, 5
        d = bz.synth.l1_quadratic(n, dtype=dtype)
        box = (bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])), ref.ClosedSet(ref.IndBox(dtype(d["lo"]), dtype(d["hi"]))))
        return n, n, (bz.DiagQuadratic(d["q"], d["b"]), bz.NormL21(12.0, K), bz.IdentityFunction(), box[0]), \
            (ref.DiagQuadratic(d["q"], d["b"]), bz.NormL21(12.0, K), ref.IdentityFunction(), box[1]), None
    if name == "dense":
        m, n, ny, K = 40, 96, 12, 3
        rng = np.random.default_rng(4)
        A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(dtype)
        b = rng.standard_normal(m).astype(dtype)
        Ac = (rng.standard_normal((ny, n)) / np.sqrt(n)).astype(dtype)
        bc = (0.1 * rng.standard_normal(ny)).astype(dtype)
        return n, ny, (bz.LeastSquares(A, b), bz.NormL21(0.3, K), bz.DenseAffine(Ac, bc), bz.ZeroSet()), \
            (ref.LeastSquares(A, b), bz.NormL21(0.3, K), ref.DenseAffine(Ac, bc), ref.ZeroSet()), None
    assert name == "sparse_ls+sparse_c"
    m, n, K = 60, 128, 4
    d = bz.synth.sparse_lasso(m, n, 5, dtype)
    f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], n)
    bb = bz.synth.budget_bands(n, 20, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    return n, 21, (f, bz.NormL21(0.5, K), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"]))), \
        (ref.LeastSquares(f.toarray(), d["b"]), bz.NormL21(0.5, K), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"]))), None


def traces(bz, ref, dev, orc, n, ny, mu, y, x0, iters, dtype, gamma):
    """tests.test_gpu_parity.run_traces with the subsolver's `gamma` / `adaptive` keywords on both sides: rows
    (k, err_x, err_z, gamma_dev, gamma_ref, g_z_dev, g_z_ref, fused, the oracle's own extended-precision envelope)"""
    eps = float(np.finfo(dtype).eps)
    kw = {} if gamma is None else {"gamma": gamma, "adaptive": True}
    prob = bz.Problem(*dev, n, ny, dtype)
    prob.set_multipliers(mu, y)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps, **kw).c_opts(), x0)
    kwr = {} if gamma is None else {"gamma": dtype(gamma), "adaptive": True}
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=eps, **kwr)
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    rows, env = [], 0.0
    for k in range(iters):
        st = sts[0]
        sc = prob.panoc_scalars()
        xd, zd = prob.panoc_vector("x"), prob.panoc_vector("z")
        env = max(env, _err(sts[1].x, st.x), _err(sts[1].z, st.z))
        rows.append((k + 1, _err(xd, st.x), _err(zd, st.z), sc["gamma"], float(st.gamma), sc["g_z"], float(st.g_z), sc["fused"], env))
        if k + 1 < iters:
            prob.panoc_step()
            sts[0] = its[0].step(sts[0])
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    return prob, rows


STATES = [("multinomial-K3", np.float64), ("multinomial-K8", np.float64), ("multinomial-K3", np.float32), ("multinomial-K8-box", np.float64),
          ("sparse_ls", np.float64), ("sparse_ls", np.float32), ("diag", np.float64), ("diag", np.float32), ("dense", np.float64),
          ("sparse_ls+sparse_c", np.float64)]


@pytest.mark.parametrize("name,dtype", STATES, ids=[f"{s[0]}-{'f64' if s[1] is np.float64 else 'f32'}" for s in STATES])
def test_iterates_follow_the_oracle(bz, ref, name, dtype):
    """30 states of the oracle's PANOCplus with the numpy class as g: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5,
    sens the oracle's own extended-precision envelope — gamma equal to 1e-12 / 1e-5 relative and g(z) to the same bound times
    the envelope rule: the rule and the numbers of tests/test_gpu_sparse_multinomial.py."""
    n, ny, dev, orc, gamma = state_problem(bz, ref, name, dtype)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    prob, rows = traces(bz, ref, dev, orc, n, ny, mu, y, x0, 30, dtype, gamma)
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
    assert pr["fb_step"]["form"].startswith("k_fbstep_group<KP="), pr["fb_step"]["form"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0 and stats.n_fused_iters == 0
    assert len({r[1] for r in rows}) > 1 or rows[-1][1] == 0.0


# ---- 4. a whole alps solve of the grouped multinomial
def test_whole_grouped_multinomial_solve(bz, ref):
    """m = 200, n_f = 30, K = 4, lambda_j = 1 with an unpenalised intercept row: the oracle zeroes 14 of the 30 rows and keeps 16
    (lambda_j = 0.6: 9 zero rows, 1.4: 20; at least a third each way is asserted on the CPU first); device and oracle agree on the status and on the set of all-zero rows,
    every penalised row is entirely zero or has no zero in it, and the intercept row is non-zero."""
    m, nf, K = 200, 30, 4
    n = nf * K
    d = bz.synth.sparse_multinomial(m, nf, K, 5, np.float64)
    f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], nf, K)
    fo = MultinomialOracle(f.toarray(), d["labels"], K, what_of(None, 1.0, np.float64))
    lam = np.full(nf, 1.0)
    lam[0] = 0.0
    g = bz.NormL21(lam, K)
    box = (bz.ClosedSet(bz.IndBox(-5.0, 5.0)), ref.ClosedSet(ref.IndBox(-5.0, 5.0)))
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, gamma=0.1, adaptive=True, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, gamma=0.1, adaptive=True, **kw)
    o = ref.alps(fo, g, ref.IdentityFunction(), box[1], np.zeros(n), np.zeros(n), subsolver=subr, subsolver_maxit=100000)
    Xo = o[0].reshape(nf, K)
    zero_o = np.all(Xo == 0, axis=1)
    assert o[5] == "first_order" and zero_o.sum() >= nf // 3 and (~zero_o).sum() >= nf // 3, (o[5], zero_o.sum())
    a = bz.alps(f, g, bz.IdentityFunction(), box[0], np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000)
    Xa = a[0].reshape(nf, K)
    zero_a = np.all(Xa == 0, axis=1)
    print(f"status {a[5]} / {o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} zero rows {zero_a.sum()}/{zero_o.sum()} "
          f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert a[5] == o[5]
    assert np.array_equal(zero_a, zero_o)
    for X in (Xa, Xo):
        nz = np.count_nonzero(X[1:], axis=1)
        assert np.all((nz == 0) | (nz == K))
        assert np.any(X[0] != 0)


# ---- 5. set_g_lambda along a path
@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
def test_lambda_path_on_a_live_problem(bz, ref, vector):
    """three values on one problem: each solve equals a fresh problem's bit for bit"""
    m, nf, K = 60, 12, 3
    n = nf * K
    d = bz.synth.sparse_multinomial(m, nf, K, 5, np.float64)
    f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], nf, K)
    rest = (bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, 5.0)))
    base = np.full(nf, 1.0)
    base[0] = 0.0
    path = [s * base if vector else s for s in (2.0, 1.0, 0.5)]
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, gamma=0.1, adaptive=True, **kw)
    live = bz.Problem(f, bz.NormL21(path[0], K), *rest, n, n, np.float64)
    sols = []
    for i, lam in enumerate(path):
        if i:
            live.set_g_lambda(lam)
        g = bz.NormL21(lam, K)
        got = bz.alps(f, g, *rest, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, problem=live)
        fresh = bz.alps(f, g, *rest, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, resident=True)
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]) and got[2:4] == fresh[2:4] and got[5] == fresh[5]
        sols.append(got[0])
    with pytest.raises(bz.BazingaHipError):
        live.set_g_lambda(base if not vector else 0.5)                 # number <-> vector stays a creation-time decision
    live.close()
    assert not np.array_equal(sols[0], sols[1]) and not np.array_equal(sols[1], sols[2])


# ---- 6. the kind changes nothing else
def test_the_kind_stays_on_the_kernel_chain_and_l1_keeps_its_form(bz, ref):
    n, K = 20011 - 1, 5
    d = bz.synth.l1_quadratic(n)
    rest = (bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
    sub = bz.PANOCplus(tol=1e-8, maxit=60)
    out = {}
    for name, g in (("group", bz.NormL21(d["lam"], K)), ("l1", bz.NormL1(d["lam"]))):
        prob = bz.Problem(bz.DiagQuadratic(d["q"], d["b"]), g, *rest, n, n, np.float64)
        prob.set_multipliers(np.full(n, 0.1), np.zeros(n))
        x, st = prob.panoc_solve(sub.c_opts(), np.zeros(n))
        out[name] = (int(st.n_fused_iters), int(st.iters), prob.profile2())
        prob.close()
    fused, iters, pr = out["group"]
    assert fused == 0 and iters > 3 and pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0
    assert pr["fb_step"]["form"] == "k_fbstep_group<KP=8,NT=0>"
    fused, iters, pr = out["l1"]
    assert fused > 0 and pr["k_fused_iterates"]["launches"] + pr["k_fused_sep"]["launches"] > 0
