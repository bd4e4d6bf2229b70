"""g = ElasticNet (BZ_G_ELASTIC_NET: l1 plus ridge with penalty factors) on the device, and l1 / l2 changed on a live problem
(bz_problem_set_g_elastic_net): creation and refusals through the raw ABI, one prox bit for bit against the numpy class and
against the closed form in extended precision, two identities with NormL1's vector form, thirty states of every path that
evaluates the prox, ALS, a closed-form minimiser, an unpenalised intercept, the setter.

The oracle side is oracle/bazinga_ref.py with the numpy bz.ElasticNet as its g.  The penalty factors are those of
tests/test_gpu_weighted_l1.py's lambda (0.5 U(0, 1) with exact zeros at the first index, the last one and one in the middle)
under l1 = 1, so the l1 half is that test's, and l2 > 0 adds the ridge."""
import ctypes as C

import numpy as np
import pytest

from tests.test_elastic_net_host import exact_prox, prox_bound
from tests.test_gpu_parity import make_cfg2, make_cfg3, make_cfg4
from tests.test_gpu_sparse import csr_of, sets, structured
from tests.test_gpu_sparse_glm import GLMOracle, glm_of, what_of
from tests.test_gpu_sparse_least_squares import CsrOracle
from tests.test_gpu_sparse_logistic import TOL
from tests.test_gpu_weighted_l1 import DT, SHAPES, assert_same_states, follow, lasso_ls, stepped, trace, with_intercept
from tests.test_weighted_l1_host import weights

pytestmark = pytest.mark.gpu

L2 = 0.3                                                       # the ridge weight of the stepping tests


def enet_pair(bz, w, l2=L2, l1=1.0):
    """(the device's g, the oracle's g): two objects of the numpy class"""
    return bz.ElasticNet(l1, l2, w), bz.ElasticNet(l1, l2, w)


# ---- 1. creation and refusals through the raw ABI
def test_creation_and_refusals_through_the_raw_abi(bz):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    n = 12
    u = np.ones(n)
    w = 2.0 * weights(n)

    def create(desc):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    def desc_of(l1, l2, wv, kind=L.BZ_G_ELASTIC_NET, dtype=np.float64):
        desc, keep = lower(bz.Zero(), bz.NormL1(1.0), bz.IdentityFunction(), bz.FreeSet(), n, n, np.dtype(dtype))
        desc.g_kind, desc.g_lambda, desc.g_l2 = kind, l1, l2
        desc.g_weights = None if wv is None else wv.ctypes.data
        return desc

    assert L.BZ_G_ELASTIC_NET == 11
    for wv in (None, w):
        assert create(desc_of(0.5, 0.25, wv))[:2] == (0, True)
        assert create(desc_of(0.0, 0.25, wv))[:2] == (0, True)          # pure ridge
        assert create(desc_of(0.5, 0.0, wv))[:2] == (0, True)           # l2 = 0
    assert create(desc_of(0.5, 0.25, w.astype(np.float32), dtype=np.float32))[:2] == (0, True)
    for bad in (-0.25, np.nan, np.inf, -np.inf):
        rc, made, msg = create(desc_of(bad, 0.25, w))
        assert rc == L.BZ_ERR_ARG and not made and "ElasticNet" in msg and "g_lambda" in msg, msg
        rc, made, msg = create(desc_of(0.5, bad, None))
        assert rc == L.BZ_ERR_ARG and not made and "ElasticNet" in msg and "g_l2" in msg, msg
    # a number that is finite in double and rounds to +inf in an fp32 problem
    w32 = w.astype(np.float32)
    rc, made, msg = create(desc_of(1e39, 0.25, w32, dtype=np.float32))
    assert rc == L.BZ_ERR_ARG and not made and "g_lambda" in msg, msg
    rc, made, msg = create(desc_of(0.5, 1e39, w32, dtype=np.float32))
    assert rc == L.BZ_ERR_ARG and not made and "g_l2" in msg, msg
    assert create(desc_of(1e39, 1e39, w))[:2] == (0, True)              # ... and is taken by an fp64 one
    for bad in (-0.25, np.nan, np.inf):
        worse = w.copy()
        worse[5] = bad
        rc, made, msg = create(desc_of(0.5, 0.25, worse))
        assert rc == L.BZ_ERR_ARG and not made and "ElasticNet" in msg and "g_weights" in msg and "entry 5" in msg, msg
    desc = desc_of(0.5, 0.25, w)
    desc.g_lambda_vec = w.ctypes.data
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "g_weights" in msg, msg
    # every other kind ignores the two fields: junk in them changes nothing
    junk = np.full(n, -np.inf)
    for kind in (L.BZ_G_NORM_L1, L.BZ_G_NORM_L1_NONNEG, L.BZ_G_NORM_L1_BOX, L.BZ_G_IND_BOX, L.BZ_G_NORM_L0_BOX,
                 L.BZ_G_NORM_LP_NONNEG, L.BZ_G_NORM_LP_BOX):
        desc = desc_of(1.0, np.nan, junk, kind)
        desc.g_u, desc.g_p, desc.g_lo, desc.g_hi = u.ctypes.data, 0.5, -1.0, 1.0
        assert create(desc)[:2] == (0, True), kind


# ---- 2. one prox, bit for bit
SPECIALS = ("nan", "+inf", "-inf", "+0", "-0", "+a", "-a")
# (name, l1, l2, weighted)
PROX_FORMS = [("number", 0.7, 0.4, False), ("weighted", 0.7, 0.4, True), ("ridge", 0.0, 0.9, True), ("l2=0", 0.6, 0.0, True)]


def special(name, a_i):
    return {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+0": 0.0, "-0": -0.0, "+a": a_i, "-a": -a_i}[name]


@pytest.mark.parametrize("form", PROX_FORMS, ids=[f[0] for f in PROX_FORMS])
@pytest.mark.parametrize("n", [1, 3, 2121])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=DT)
def test_one_prox_bit_for_bit(bz, dtype, n, form):
    """z bit-equal to bz.ElasticNet.prox (zeros compared with their signs, the NaN pattern equal), g(z) inside TOL of the float64
    sum of the terms; and the same z against soft(y, gamma w l1) / (1 + gamma w l2) in np.longdouble with the host test's bound
    8 eps (|y| + a) + the smallest normal, which does not go through the restated class.  Shorter than the three zeros of the
    weights' rule (n = 1, 3) a draw without zeros is run as well."""
    name, l1, l2, weighted = form
    gamma = 0.37
    draws = [2.0 * weights(n, 4)] + ([np.random.default_rng(4).uniform(0.0, 1.0, n)] if n < 5 else [])
    for w in (draws if weighted else [None]):
        g = bz.ElasticNet(l1, l2, w)
        prob = bz.Problem(bz.Zero(), g, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
        a = (dtype(gamma) * (np.ones(n, dtype) if w is None else w.astype(dtype))) * dtype(l1)
        rng = np.random.default_rng(5)
        xs = []
        if n >= 64:
            x = (0.3 * rng.standard_normal(n)).astype(dtype)
            # every special at a positive weight, at a zero weight (index 0, the middle one, the last) and in the ragged last pack
            for j, sp in enumerate(SPECIALS):
                for i in (7 + j, n - 9 + j):
                    x[i] = special(sp, a[i])
            xs.append(x)
            for j, sp in enumerate(SPECIALS):
                x = (0.3 * rng.standard_normal(n)).astype(dtype)
                x[[0, n // 2, n - 1]] = [special(SPECIALS[(j + k) % 7], a[i]) for k, i in enumerate((0, n // 2, n - 1))]
                xs.append(x)
        else:
            for j, sp in enumerate(SPECIALS):
                x = (0.3 * rng.standard_normal(n)).astype(dtype)
                x[j % n] = special(sp, a[j % n])
                xs.append(x)
        xs.append((0.3 * rng.standard_normal(n)).astype(dtype))           # finite: the value
        for x in xs:
            zr = np.empty(n, dtype)
            with np.errstate(invalid="ignore"):
                vr = float(g.prox(zr, x, gamma))
            zd, vd = prob.eval_prox(x, gamma)
            assert zd.dtype == dtype
            assert np.array_equal(np.isnan(zd), np.isnan(zr))
            assert np.array_equal(zd, zr, equal_nan=True), (x, zd, zr)
            assert np.array_equal(np.signbit(zd[zd == 0]), np.signbit(zr[zr == 0]))
            # the closed form in extended precision, where y is finite
            fin = np.isfinite(x)
            zs, al = exact_prox(x[fin], gamma, l1, l2, None if w is None else w[fin], dtype)
            err, bound = np.abs(zd[fin].astype(np.longdouble) - zs), prox_bound(x[fin], al, dtype)
            assert np.all(err <= bound), float(np.max(err / bound))
            if np.isfinite(vr):
                z64 = zr.astype(np.float64)
                terms = float(dtype(l1)) * np.abs(z64) + 0.5 * float(dtype(l2)) * z64 * z64
                scale = float(np.sum(terms if w is None else w.astype(dtype).astype(np.float64) * terms))
                print(f"{name} n={n} g(z) {vd:.17g} / {vr:.17g} / {scale:.17g} worst |z - z*| / bound {float(np.max(err / bound)):.3f}")
                assert abs(vd - scale) <= TOL[dtype] * scale
            else:
                assert (np.isnan(vd) and np.isnan(vr)) or vd == vr
        prob.close()


# ---- 3. two identities with NormL1's vector form
@pytest.mark.parametrize("which", ["l2=0", "l1=1,weights"])
def test_identities_with_the_weighted_l1(bz, ref, which):
    """ElasticNet(l1, 0) is NormL1(full(n, l1)) and ElasticNet(1, 0, weights=v) is NormL1(v), bit for bit in every state: with
    l2 = 0 the divisor is 1 + t * 0 = 1, s / 1 = s and the ridge term adds +0; t * 1 = t.  Both run the same run-time forms."""
    n = 2121
    d, dev, orc = make_cfg2(bz, ref, n)
    mu, y = np.full(n, 0.1), 0.1 * np.random.default_rng(2).standard_normal(n)
    x0 = np.zeros(n)
    if which == "l2=0":
        l1 = float(d["lam"])
        ga, gb = bz.ElasticNet(l1, 0.0), bz.NormL1(np.full(n, l1))
    else:
        v = weights(n, 6)
        ga, gb = bz.ElasticNet(1.0, 0.0, v), bz.NormL1(v)
    a, pra = stepped(bz, (dev[0], ga) + dev[2:], n, n, np.float64, x0, 30, mu, y)
    b, prb = stepped(bz, (dev[0], gb) + dev[2:], n, n, np.float64, x0, 30, mu, y)
    assert_same_states(a, b)
    assert any(np.any(x != 0) for x, _, _ in a)
    assert {c: pra[c]["launches"] for c in pra} == {c: prb[c]["launches"] for c in prb}          # the same kernels
    assert {c: pra[c]["form"] for c in pra} == {c: prb[c]["form"] for c in prb}
    assert pra["k_fused_sep"]["form"].startswith("k_fused_compact<XR=0,SPEC=0"), pra["k_fused_sep"]["form"]
    assert pra["k_fused_sep"]["launches"] > 0 and pra["k_fused_iterates"]["launches"] == 0


# ---- 4. thirty states follow the oracle
def setup_diag(bz, ref, dtype):
    n = 2121
    d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
    gd, gr = enet_pair(bz, weights(n, 6))
    return n, n, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


def setup_sparse_ls(bz, ref, dtype, beside_c=False):
    A, b, (indptr, indices, data), rng = with_intercept(SHAPES[0], dtype)
    n = A.shape[1]
    gd, gr = enet_pair(bz, weights(n, 7))
    f, fo = bz.SparseLeastSquares(indptr, indices, data, b, n), ref.LeastSquares(A, b)
    Dd, Dr = sets(bz, ref, "box", dtype)
    if not beside_c:
        return n, n, (f, gd, bz.IdentityFunction(), Dd), (fo, gr, ref.IdentityFunction(), Dr)
    ny = 30
    Ac = structured(ny, n, 0.2, rng, False, dtype)
    bc = rng.standard_normal(ny).astype(dtype)
    csr = csr_of(Ac, np.random.default_rng(3)) + (bc, n)
    return n, ny, (f, gd, bz.SparseAffine(*csr), Dd), (fo, gr, CsrOracle(*csr), Dr)


def setup_glm(bz, ref, dtype, data_seed=0):
    m, n, p = SHAPES[0]
    rng = np.random.default_rng(m * 13 + n + data_seed)
    A = structured(m, n, p, rng, False, dtype)
    b = np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)
    w = (0.5 + rng.random(m)).astype(dtype)
    f = glm_of(bz, A, b, "logistic", None, w, 1.0 / m)[0]
    fo = GLMOracle(f.toarray(), b, "logistic", None, what_of(w, 1.0 / m, dtype))
    gd, gr = enet_pair(bz, weights(n, 8) / m)
    Dd, Dr = sets(bz, ref, "box", dtype)
    return n, n, (f, gd, bz.IdentityFunction(), Dd), (fo, gr, ref.IdentityFunction(), Dr)


def setup_stencil(bz, ref, dtype):
    nx, ny = 12, 14
    d, n, dev, orc = make_cfg3(bz, ref, nx, ny)
    gd, gr = enet_pair(bz, weights(n, 9) * float(np.max(np.abs(dev[0].b))))
    return n, n, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


def setup_dense(bz, ref, dtype):
    ny, n = 5, 12                                              # the smallest shape of tests/test_gpu_dense.py
    d, dev, orc = make_cfg4(bz, ref, ny, n, dtype, density=0.5)
    gd, gr = enet_pair(bz, 2.0 * weights(n, 10))
    return n, ny, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


def setup_of(bz, ref, which, dtype, data_seed):
    return {"diag": setup_diag, "sparse-ls": setup_sparse_ls, "sparse-ls+c": lambda *a: setup_sparse_ls(*a, beside_c=True),
            "glm": lambda *a: setup_glm(*a, data_seed=data_seed), "stencil": setup_stencil, "dense": setup_dense}[which](bz, ref, dtype)


# (set-up, dtype, the seed of y, the draw of the GLM's data): every set-up in fp64, and in fp32 all but the stencil, whose
# generator (make_cfg3) is fp64 alone, as in tests/test_gpu_weighted_l1.py.  Seeds were chosen on the oracle alone (its two
# reducers, no device), so that at least 25 (fp64) / 8 (fp32) states are held to `base`.  Seed 2, the first tried, did for seven
# (30 states in fp64; 14 and 8 in fp32: the count saturates at 8 for the fp32 sparse least squares, seeds 2 .. 15 give 6 to 8);
# seed 3 for sparse-ls+c fp32 (6 -> 11), the GLM in fp64 (11 -> 30) and dense fp32 (11 -> 16).
# The fp32 logistic GLM needs a second condition.  `sens` is the oracle's sensitivity to the ORDER of its sums; the fp32
# logistic step can be as sensitive to the last bits of exp / log1p, in which a device legitimately differs from numpy and
# which `sens` does not see.  On the oracle alone, with l'(b, t) moved by -1, 0 or +1 fp32 ulp at random rows, two oracle runs
# of data draw 0, seed 3 (13 states held) are 1.1e-7 apart at state 6 and 2.0e-4 at state 7: 75 times the rule's bound.  So
# data draws 0 .. 7 x seeds 2 .. 9 were searched, still on the oracle alone, for at least 8 states held AND every one of 30
# states of eight such perturbed runs inside max(base, 100 sens).  14 of the 64 hold 8 states or more; of these nine leave the
# bound (by 1.5 to 225 times) and five stay inside: (3, 9) at 0.56 of the bound, (5, 6) 0.11, (5, 7) 0.06, (6, 8) 0.02,
# (7, 2) 0.08.  Those were run again with perturbations of up to 2 and up to 4 ulps (twelve runs each): (5, 6) and (5, 7) leave
# the bound at 2 ulps (3.3 and 11.5 times), (7, 2) stays at 0.13, (6, 8) at 0.04.  The case is the steadiest: data draw 6, seed 8.
FOLLOW = [("diag", np.float64, 2, 0), ("diag", np.float32, 2, 0), ("sparse-ls", np.float64, 2, 0), ("sparse-ls", np.float32, 2, 0),
          ("sparse-ls+c", np.float64, 2, 0), ("sparse-ls+c", np.float32, 3, 0), ("glm", np.float64, 3, 0), ("glm", np.float32, 8, 6),
          ("stencil", np.float64, 2, 0), ("dense", np.float64, 2, 0), ("dense", np.float32, 3, 0)]


@pytest.mark.parametrize("which,dtype,seed,data_seed", FOLLOW, ids=[f"{w}-{DT(t)}" for w, t, _, _ in FOLLOW])
def test_thirty_states_follow_the_oracle(bz, ref, which, dtype, seed, data_seed):
    n, ny, dev, orc = setup_of(bz, ref, which, dtype, data_seed)
    assert np.count_nonzero(dev[1].weights == 0) >= 3 and dev[1].l2 > 0
    pr = follow(bz, ref, dev, orc, n, ny, dtype, seed)
    forms = {c: (pr[c]["form"], pr[c]["launches"]) for c in pr if pr[c]["launches"]}
    print(forms)
    # the host keeps this g out of the family kernels (and of every other iterate-history pass)
    assert pr["k_fused_iterates"]["launches"] == 0, pr["k_fused_iterates"]
    assert pr["fb_step"]["launches"] > 0                                                        # k_fbstep
    if which == "diag":
        assert pr["k_fused_sep"]["form"].startswith("k_fused_compact<XR=0,SPEC=0"), pr["k_fused_sep"]["form"]
        assert pr["k_fused_sep"]["launches"] > 0
    if which.startswith("sparse") or which == "glm":
        assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
    if which == "stencil":
        assert pr["k_stencil_fb"]["launches"] > 0
    if which == "dense":
        assert pr["gemv"]["launches"] > 0


# ---- 5. ALS
def als_case(bz, ref, which):
    nx = 100
    q, fb = 0.5 + bz.synth.uniform(1, nx), 2 * bz.synth.uniform(2, nx) - 1
    w = 0.2 * weights(nx, 11)
    gd, gr = enet_pair(bz, w)
    obj = lambda x: float(np.sum(x * (0.5 * q * x - fb)) + gd(x))
    if which == "identity":
        dev = (bz.DiagQuadratic(q, fb), gd, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
        orc = (ref.DiagQuadratic(q, fb), gr, ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(-0.1, 0.2)))
        return nx, nx, dev, orc, obj, lambda x: x
    ny = 20
    d = bz.synth.basis_pursuit(ny, nx, dtype=np.float64, density=0.05)
    dev = (bz.DiagQuadratic(q, fb), gd, bz.DenseAffine(d["A"], d["b"]), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
    orc = (ref.DiagQuadratic(q, fb), gr, ref.DenseAffine(d["A"], d["b"]), ref.ClosedSet(ref.IndBox(-0.1, 0.2)))
    return nx, ny, dev, orc, obj, lambda x: d["A"] @ x - d["b"]


@pytest.mark.parametrize("which", ["identity", "dense"])
def test_als_against_the_oracle(bz, ref, which):
    """the comparison of test_als_against_the_oracle in tests/test_gpu_weighted_l1.py (that of test_whole_solves in
    tests/test_gpu_als_dense.py), with its bounds; the one-pass slack forms run, the fast ones are not taken"""
    nx, ny, dev, orc, obj, cfun = als_case(bz, ref, which)
    sub_kw = dict(maxit=100000, minimum_gamma=2.3e-16)
    x0 = np.zeros(nx)
    o = ref.als(*orc, x0.copy(), np.zeros(ny), subsolver=lambda **k: ref.PANOCplus(**sub_kw, **k), subsolver_maxit=100000)
    assert o[5] == "first_order"
    prob = bz.Problem(*dev, nx, ny, np.float64, slack=True)
    a = bz.als(*dev, x0, np.zeros(ny), subsolver=lambda **k: bz.PANOCplus(**sub_kw, **k), subsolver_maxit=100000, problem=prob)
    pr = prob.profile2()
    prob.close()
    cx = cfun(a[0])
    feas = float(np.max(np.abs(cx - np.clip(cx, -0.1, 0.2))))
    print(f"{which}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} obj {obj(a[0]):.9g}/{obj(o[0]):.9g} "
          f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e} forms {pr['k_fused_iterates']['form']!r} {pr['k_fused_sep']['form']!r}")
    assert a[5] == "first_order"
    assert feas <= 1e-5
    assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    assert np.max(np.abs(a[8] - np.clip(a[8], -0.1, 0.2))) == 0.0
    assert "fast" not in pr["k_fused_iterates"]["form"] and "fast" not in pr["k_fused_sep"]["form"]
    if which == "identity":
        seen = [pr[c]["form"] for c in ("k_fused_iterates", "k_fused_sep") if pr[c]["launches"] > 0]
        assert seen and all(s.startswith("k_fused_slack") for s in seen), seen          # (the run-time one-pass slack forms)
    else:
        # (unequal halves have no one-pass form: the lifted kernel chain, whose step is k_fbstep_lifted)
        assert pr["fb_step"]["form"].startswith("k_fbstep_lifted<LP=0>") and pr["fb_step"]["launches"] > 0, pr["fb_step"]


# ---- 6. a closed form, independent of the class
def test_closed_form_minimiser(bz, ref):
    """f = DiagQuadratic(q, b), c = Identity, D = FreeSet: the augmented Lagrangian is f itself (the distance to the free set is
    zero), and F = f + g is separable with F_i(x) = q_i x^2 / 2 - b_i x + w_i (l1 |x| + l2 x^2 / 2), minimised at
    x*_i = soft(b_i, w_i l1) / (q_i + w_i l2).

    The bound.  PANOCplus returns z = prox_{gamma g}(x - gamma grad f(x)) once
    ||v||_inf <= tol, v = (x - z) / gamma - grad f(x) + grad f(z).  By the prox's optimality, (x - gamma grad f(x) - z) / gamma is
    a subgradient of g at z, so v is a subgradient of F at z, element for element: v_i in dF_i(z_i), and 0 in dF_i(x*_i).
    F_i is strongly convex with modulus q_i + w_i l2 >= q_i, so (v_i - 0) (z_i - x*_i) >= q_i (z_i - x*_i)^2, hence
    |z_i - x*_i| <= |v_i| / q_i <= tol / min q.  alps ends only after an inner solve at inner_tol <= tol_dual = tol.
    v is evaluated in floating point: its three terms are each at most max(|b|, |q x|) <= 2 max|b| in size here and each is
    rounded a few times, which moves v by less than 16 eps max|b|; that is added to tol.  With tol = 1e-8, q in [0.5, 2]:
    max |z - x*| <= (1e-8 + 16 eps max|b|) / min q, about 2e-8.  The oracle's alps is held to it first, then the device."""
    n = 2121
    rng = np.random.default_rng(21)
    q, b = rng.uniform(0.5, 2.0, n), 2.0 * rng.standard_normal(n)
    w = 2.0 * weights(n, 22)
    l1, l2, tol = 0.8, 0.6, 1e-8
    xstar = np.sign(b) * np.maximum(np.abs(b) - w * l1, 0.0) / (q + w * l2)
    assert np.count_nonzero(xstar) > n // 4 and np.count_nonzero(xstar == 0) > n // 8
    bound = (tol + 16 * np.finfo(np.float64).eps * float(np.max(np.abs(b)))) / float(np.min(q))
    gd, gr = enet_pair(bz, w, l2, l1)
    dev = (bz.DiagQuadratic(q, b), gd, bz.IdentityFunction(), bz.FreeSet())
    orc = (ref.DiagQuadratic(q, b), gr, ref.IdentityFunction(), ref.FreeSet())
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(n), subsolver=subr, subsolver_maxit=100000, tol=tol)
    a = bz.alps(*dev, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, tol=tol)
    eo, ea = float(np.max(np.abs(o[0] - xstar))), float(np.max(np.abs(a[0] - xstar)))
    print(f"status {a[5]} / {o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} max|x - x*| {ea:.3e} / {eo:.3e} bound {bound:.3e}")
    assert o[5] == "first_order" and eo <= bound
    assert a[5] == "first_order" and ea <= bound
    assert np.array_equal(a[0] == 0, xstar == 0)


# ---- 7. an unpenalised intercept
def test_intercept_is_unpenalised(bz, ref):
    """the 257 x 1031 least squares of tests/test_gpu_weighted_l1.py with a column of ones, glmnet's penalty with
    penalty_factor 0 there and 1 elsewhere, at a lambda that zeroes every penalised coefficient: with x_j = 0 for the penalised
    j the intercept is mean(b), and that point is the minimiser when lambda alpha >= max_j |A_j' (b - mean(b))| (the
    subgradient condition at zero); lambda alpha is 1.05 times that.  The device follows ref.alps within 1e-4 (that test's bound,
    both sides at tol = 1e-8 as there), the penalised coefficients are exactly zero and the intercept is not."""
    A, b, (indptr, indices, data), rng = with_intercept(SHAPES[1], np.float64)
    m, n = A.shape
    assert np.all(A[:, n - 1] == 1.0)
    pf = np.ones(n)
    pf[n - 1] = 0.0
    alpha = 0.5
    lam = 1.05 * float(np.max(np.abs(A[:, :n - 1].T @ (b - np.mean(b))))) / alpha
    gd, gr = bz.ElasticNet.glmnet(lam, alpha, pf), bz.ElasticNet.glmnet(lam, alpha, pf)
    dev = (bz.SparseLeastSquares(indptr, indices, data, b, n), gd, bz.IdentityFunction(), bz.FreeSet())
    orc = (ref.LeastSquares(A, b), gr, ref.IdentityFunction(), ref.FreeSet())
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(n), subsolver=subr, subsolver_maxit=100000, tol=1e-8)
    a = bz.alps(*dev, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, tol=1e-8)
    grad = A.T @ (A @ a[0] - b)
    print(f"status {a[5]} / {o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} inner_tol {a[6]:.3e} |grad_intercept| {abs(grad[n - 1]):.3e} "
          f"x_intercept {a[0][n - 1]:.9g} / {o[0][n - 1]:.9g} mean(b) {np.mean(b):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert o[5] == "first_order" and a[5] == "first_order"
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    assert abs(grad[n - 1]) <= 10 * a[6]
    assert np.all(a[0][:n - 1] == 0.0) and a[0][n - 1] != 0.0
    assert np.all(o[0][:n - 1] == 0.0)


# ---- 8. the setter
@pytest.mark.parametrize("weighted", [False, True], ids=["number", "weighted"])
def test_set_g_elastic_net_equals_a_fresh_problem(bz, weighted):
    n, f, rest, mu, y = lasso_ls(bz)
    w = 2.0 * weights(n, 13) if weighted else None
    (l1a, l2a), (l1b, l2b) = (0.4, 0.3), (0.15, 0.7)
    x0 = (0.1 * np.random.default_rng(3).standard_normal(n))
    held = {}

    def before(prob):
        held["first"] = trace(bz, prob, x0, 20)                # a solve at the first pair on the same problem
        prob.set_g_elastic_net(l1b, l2b)
    a, _ = stepped(bz, (f(), bz.ElasticNet(l1a, l2a, w)) + rest, n, n, np.float64, x0, 20, mu, y, before)
    b, _ = stepped(bz, (f(), bz.ElasticNet(l1b, l2b, w)) + rest, n, n, np.float64, x0, 20, mu, y)
    assert_same_states(a, b)
    assert not np.array_equal(held["first"][-1][1], a[-1][1])  # ... and the first pair gave something else


def test_a_path_on_one_problem_equals_fresh_problems(bz):
    """five lambda of a glmnet path (alpha = 0.6, penalty factors with an unpenalised intercept) on one problem, each a traced
    solve of 12 steps from the same x0: every state equals that of a problem created at that lambda"""
    n, f, rest, mu, y = lasso_ls(bz)
    pf = np.ones(n)
    pf[n - 1] = 0.0
    alpha = 0.6
    x0 = (0.1 * np.random.default_rng(4).standard_normal(n))
    lams = [2.0, 1.0, 0.5, 0.25, 0.125]
    prob = bz.Problem(f(), bz.ElasticNet.glmnet(lams[0], alpha, pf), *rest, n, n, np.float64)
    prob.set_multipliers(mu, y)
    ends = []
    for k, lam in enumerate(lams):
        if k:
            prob.set_g_elastic_net(lam * alpha, lam * (1 - alpha))
        on_path = trace(bz, prob, x0, 12)
        fresh, _ = stepped(bz, (f(), bz.ElasticNet.glmnet(lam, alpha, pf)) + rest, n, n, np.float64, x0, 12, mu, y)
        assert_same_states(on_path, fresh)
        ends.append(on_path[-1][1])
    prob.close()
    assert all(not np.array_equal(ends[k], ends[k + 1]) for k in range(4))


def test_set_g_elastic_net_refusals(bz):
    L = bz._lib
    lib = L.load()
    n, f, rest, mu, y = lasso_ls(bz)
    w = 2.0 * weights(n, 15)
    x0 = np.zeros(n)
    set_raw = lambda prob, l1, l2: (lib.bz_problem_set_g_elastic_net(prob._h, l1, l2), lib.bz_last_error().decode())
    wp = bz.Problem(f(), bz.ElasticNet(0.4, 0.3, w), *rest, n, n, np.float64)
    nump = bz.Problem(f(), bz.ElasticNet(0.4, 0.3), *rest, n, n, np.float64)
    l1p = bz.Problem(f(), bz.NormL1(0.5), *rest, n, n, np.float64)
    p32 = bz.Problem(f(), bz.ElasticNet(0.4, 0.3), *rest, n, n, np.float32)
    for prob in (wp, nump, l1p):
        prob.set_multipliers(mu, y)
    sub = bz.PANOCplus(tol=0.0, maxit=10 ** 9)
    # between begin and finish
    for prob in (wp, nump):
        prob.panoc_begin(sub.c_opts(), x0)
        prob.panoc_step()
        rc, msg = set_raw(prob, 0.2, 0.1)
        assert rc == L.BZ_ERR_STATE and "bz_panoc_finish" in msg, msg
        prob.panoc_finish()
        assert set_raw(prob, 0.4, 0.3)[0] == 0
    # any other g kind
    rc, msg = set_raw(l1p, 0.2, 0.1)
    assert rc == L.BZ_ERR_ARG and "ElasticNet" in msg, msg
    # bad numbers, each named
    for bad in (-0.5, np.nan, np.inf):
        rc, msg = set_raw(wp, bad, 0.1)
        assert rc == L.BZ_ERR_ARG and "g_lambda" in msg, msg
        rc, msg = set_raw(wp, 0.2, bad)
        assert rc == L.BZ_ERR_ARG and "g_l2" in msg, msg
    assert set_raw(p32, 1e39, 0.1)[0] == L.BZ_ERR_ARG and set_raw(p32, 0.2, 1e39)[0] == L.BZ_ERR_ARG
    # bz_problem_set_g_lambda stays refused on this kind, with its text
    rc = lib.bz_problem_set_g_lambda(wp._h, 0.25, None)
    assert rc == L.BZ_ERR_ARG and "g must be NormL1, NormL1Nonneg, NormL1Box or NormL0Box" in lib.bz_last_error().decode()
    # a refused call changes nothing: the problem still runs on (0.4, 0.3, w)
    z1, g1 = wp.eval_prox(np.full(n, 0.9), 1.0)
    fresh = bz.Problem(f(), bz.ElasticNet(0.4, 0.3, w), *rest, n, n, np.float64)
    z2, g2 = fresh.eval_prox(np.full(n, 0.9), 1.0)
    assert np.array_equal(z1, z2) and g1 == g2
    with pytest.raises(bz.BazingaHipError) as ei:
        l1p.set_g_elastic_net(0.2, 0.1)
    assert ei.value.code == L.BZ_ERR_ARG
    for prob in (wp, nump, l1p, p32, fresh):
        prob.close()
