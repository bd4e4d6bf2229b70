"""The Lp-power prox (NormLpPowerNonneg / NormLpPowerBox, lp_prox in csrc/bz_kernels.h) against an exact prox: the table
of arguments, an extended-precision twin of the prox, the two bounds the device is held to, and the proofs — on the twin
and the oracle alone, no GPU — that every expectation of tests/test_gpu_lp_prox.py is reachable.

The problem, per element:  min over z >= 0 [z <= u] of  phi(z) = a z^p + (z - x)^2 / 2,  a = alpha * gamma, 0 < p < 1.
phi'(z) = z - x + a p z^(p-1) is convex with its minimum at zbar = (a p (1 - p))^(1/(2-p)); for x > psi(zbar) = zbar +
a p zbar^(p-1) it has two roots and the larger, z*, is a local minimum of phi.  The prox is the better of 0 and
min(z*, u).  z* beats 0 exactly when x > x_t = z_t + a p z_t^(p-1), z_t = (2 a (1 - p))^(1/(2-p)): there phi(z_t) =
phi(0), and z* >= z_t for every kept element.

THE TWIN bisects phi' on [zbar, x] in np.longdouble and compares phi values; it shares no code with the oracle's Newton
loop.  It works on the arguments as the device holds them: T(p), T(gamma) * T(alpha) formed in T, T(x), T(u), widened.

THE BOUND ON z.  For z >= z_t:  phi''(z) = 1 - a p (1 - p) z^(p-2) >= 1 - p/2 > 1/2, so |z - z*| <= 2 |phi'(z)|.  The
loop ends at |phi'| <= 1e-12 in the working type or, where that is below the rounding of phi' itself, once the computed
phi' stops falling.  The computed phi' = fl(fl(z - x) + fl(fl(a p) * pow(z, fl(p - 1)))) differs from the exact one by at
most  [1/2 + 1/2 + 1/2 + 1/2 + POW_ULP + |ln z| |p - 1| / 2] eps (x + z):  the difference, the sum, the product a p, the
product with the power, the power itself by the ulp bound its library documents (16 ulp, the OpenCL bound the device
library implements; the host's is below 1), and the rounding of the exponent p - 1, which moves z^(p-1) by |ln z| times
its own relative error.  Both terms of phi' are at most x + z near the root.  Hence
    stop(x, z) = max(1e-12, C(z) eps (x + z)),  C(z) = POW_ULP + 2 + |ln z| / 2,
    |z - z*| <= 2 stop + 2 eps z        (the last step's own rounding and the final subtraction),
derived from the operations, not fitted.  Largest measured error / bound over the table: the oracle fp64 0.60, fp32 0.10
(printed by test_oracle_meets_the_bounds_over_the_table); the device fp64 0.60, fp32 0.09 in each of the three kernels
(NEXT.md).

THE DECISION MARGIN.  The kernel decides by  phi0 <= 0.5 dz^2 + a z^p  in the working type with phi0 = 0.5 x^2.  Each
side is at most 0.5 x^2 near a tie; the roundings are 1/2 eps on phi0, 3/2 eps on 0.5 dz^2 (dz, its square, the half is
exact), (POW_ULP + 1) eps on a z^p <= 0.5 x^2, 1/2 eps on the sum: below (POW_ULP / 2 + 2) eps x^2 = 10 eps x^2.  The
table uses C_MARGIN = 16: an entry whose margin |phi(0) - phi(min(z*, u))| in the twin is at most 16 eps x^2 is UNSETTLED
and either candidate is accepted for it, each within the bound on z; every other entry must have the twin's support
exactly.  The margin grows with slope z* in x, so x = x_t (1 +- k eps) is settled once k z_t > 16 x_t, i.e.
k > 16 (1 + p / (2 (1 - p))): 17 at p = 0.1, 88 at p = 0.9, 808 at p = 0.99.  The threshold rows use k in K_LIST; those
with k >= 256 (k >= 1024 at p = 0.99) are proved settled below, those with k <= 8 are unsettled on purpose.

THE VALUE OF g is compared with alpha * sum z^p in long double over the device's own z; every term is >= 0, so the bound
is (ceil(log2 n) + POW_ULP + 2) eps of the sum (a tree or fp64 sum, the power, the conversion of the sum and the product
with alpha).

THE alpha = 0 CORNER.  The classes accept alpha = 0, where the prox is min(x, u) for x > 0.  The loop gets there in one
step z = z0 - (z0 - x), which is x up to the rounding of z0 - x (half an ulp of z0 <= 1.1; a second step repairs it where
that is above 1e-12, so fp32 returns min(x, u) bit for bit and fp64 within half an ulp of max(z0, x)).  A tiny positive x (below eps / 4: 6e-17
in fp64, 3e-8 in fp32; an eighth of that for the Box kind, whose start is 0.1) makes that step land on
z = 0, 0 * pow(0, p - 1) is NaN and the prox returns NaN where the right value is x (clamped to u).  The reference does the
same; the oracle and the device keep it, and the GPU test holds the device to the oracle's bits on these rows.
"""
import functools
import math

import numpy as np
import pytest

from oracle import bazinga_ref as ref

LD = np.longdouble
POW_ULP = 16.0
C_MARGIN = 16.0
P_TABLE = (0.1, 0.3, 0.5, 2.0 / 3.0, 0.9, 0.99)
ALPHAS = (0.8, 0.0)
GAMMAS = (1.25e-6, 1.25e-3, 0.37, 12.5, 1250.0)          # alpha * gamma = 1e-6 ... 1e3 with alpha = 0.8
GAMMA_A0 = (0.37,)                                        # alpha = 0: gamma does not enter
TYPES = ("float64", "float32")
KINDS = ("nonneg", "box")
K_LIST = (1, 8, 256, 1024, 4096, 65536)
EDGE_LEN = 26                                             # the edge entries at the head of a block
BLOCK_LEN = 515                                           # entries of a row's block; no multiple of a pack (2 or 4)
SEED = 20260


def gammas_of(alpha):
    return GAMMAS if alpha > 0 else GAMMA_A0


def k_needed(p):
    return C_MARGIN * (1.0 + p / (2.0 * (1.0 - p)))


def k_settled(p):
    """the k of K_LIST from which a threshold row must be settled: the k the slope argument asks for, and 2 more for the
    rounding of x_t (1 +- k eps) into the working type"""
    return min(k for k in K_LIST if k >= k_needed(p) + 2)


def held(p, alpha, gamma, dtype):
    """(p, a = alpha * gamma) as the device holds them, widened"""
    T = np.dtype(dtype).type
    return LD(T(p)), LD(T(gamma) * T(alpha))


# ---------------------------------------------------------------------------------------------- the twin (long double)
def _phi(z, x, p, a):
    with np.errstate(all="ignore"):
        return a * z ** p + LD(0.5) * (z - x) ** 2


def _dphi(z, x, p, a):
    with np.errstate(all="ignore"):
        return z - x + a * p * z ** (p - 1)


def _bisect(f, lo, hi):
    """the point where f changes sign on [lo, hi] (f(lo) and f(hi) of opposite signs), to the last bit"""
    lo, hi = lo.copy(), hi.copy()
    up = f(hi) > 0
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if np.all((mid == lo) | (mid == hi)):
            break
        right = (f(mid) > 0) == up
        hi = np.where(right, mid, hi)
        lo = np.where(right, lo, mid)
    return hi


def stationary(xl, p, a):
    """z*, the larger root of phi', per element of xl > 0 (long double); NaN where there is none"""
    out = np.full(xl.shape, np.nan, LD)
    if a == 0:
        return xl.copy()
    zbar = (a * p * (1 - p)) ** (1 / (2 - p))
    ok = _dphi(zbar, xl, p, a) < 0
    if np.any(ok):
        x = xl[ok]
        out[ok] = _bisect(lambda z: _dphi(z, x, p, a), np.full(x.shape, zbar, LD), x)
    return out


def twin(x, u, p, a):
    """The exact prox of the arguments x (and u, or None) held in the working type, p and a widened (held()).
    Returns (z, cand, margin): the prox, the nonzero candidate min(z*, u) (0 where there is none) and |phi(0) - phi(cand)|
    (inf where there is no choice to make).  A NaN u is no bound (it passes the kernel's u == 0 and z > u tests as +inf
    does).  Entries with a non-finite x come back as NaN: they are compared with the oracle's pattern, not with this."""
    xl = np.asarray(x).astype(LD)
    n = xl.shape[0]
    z, cand, margin = np.zeros(n, LD), np.zeros(n, LD), np.full(n, np.inf, LD)
    pos = np.isfinite(xl) & (xl > 0)
    zs = np.full(n, np.nan, LD)
    if np.any(pos):
        zs[pos] = stationary(xl[pos], p, a)
    have = pos & np.isfinite(zs)
    c = np.where(have, zs, 0)
    if u is not None:
        ul = np.asarray(u).astype(LD)
        ul = np.where(np.isnan(ul), np.inf, ul)
        c = np.minimum(c, ul)
    have &= c > 0
    phic, phi0 = _phi(c, xl, p, a), LD(0.5) * xl * xl
    keep = have & (phic < phi0)
    z = np.where(keep, c, 0)
    cand = np.where(have, c, 0)
    with np.errstate(all="ignore"):
        margin = np.where(have, np.abs(phi0 - phic), np.inf)
    z = np.where(np.isfinite(xl), z, np.nan)
    return z, cand, margin


def threshold(p, a):
    """(z_t, x_t, zbar, psi(zbar)) in long double"""
    z_t = (2 * a * (1 - p)) ** (1 / (2 - p))
    x_t = z_t + a * p * z_t ** (p - 1)
    zbar = (a * p * (1 - p)) ** (1 / (2 - p))
    return z_t, x_t, zbar, zbar + a * p * zbar ** (p - 1)


def tie_bound(xl, zs, p, a):
    """u_c in (0, z*) with phi(u_c) = phi(0), per element with a kept z* (phi(z*) < phi(0)): phi - phi(0) is positive
    right of 0, negative at z*, and changes sign once between"""
    phi0 = LD(0.5) * xl * xl
    return _bisect(lambda v: -(_phi(v, xl, p, a) - phi0), np.zeros(xl.shape, LD), zs)


# ---------------------------------------------------------------------------------------------- the two bounds
def bound_z(x, cand, dtype):
    """2 stop(x, z) + 2 eps z (module docstring), in long double; 0 where the candidate is 0"""
    eps = LD(np.finfo(dtype).eps)
    xl, zl = np.abs(np.asarray(x).astype(LD)), np.asarray(cand).astype(LD)
    with np.errstate(all="ignore"):
        lnz = np.where(zl > 0, np.abs(np.log(np.where(zl > 0, zl, 1))), 0)
    stop = np.maximum(LD(1e-12), (POW_ULP + 2 + lnz / 2) * eps * (xl + zl))
    return np.where(zl > 0, 2 * stop + 2 * eps * zl, 0)


def unsettled(x, margin, dtype):
    xl = np.asarray(x).astype(LD)
    return np.isfinite(margin) & (margin <= C_MARGIN * LD(np.finfo(dtype).eps) * xl * xl)


def judged(x, dtype):
    """the entries held to the twin: a finite x whose square the working type holds (phi(0) = x^2 / 2 of the largest finite
    number overflows in the kernel; that entry is compared with the oracle's pattern, like NaN and the infinities)"""
    xl = np.asarray(x).astype(LD)
    return np.isfinite(xl) & (np.abs(xl) < LD(np.sqrt(np.finfo(dtype).max)) / 2)


def judge(z_got, x, tw, dtype, hold=None):
    """Hold z_got (working type) to the twin tw = (z, cand, margin) on the entries with a finite x (and, given hold, on
    those of that mask alone).
    Returns (bad, ratio, uns): indices that break the rule, the largest |z_got - z| / bound over the entries held to a
    nonzero value, and the mask of unsettled entries."""
    z, cand, margin = tw
    fin = judged(x, dtype)
    if hold is not None:
        fin = fin & hold
    uns = unsettled(x, margin, dtype) & fin
    b = bound_z(x, cand, dtype)
    g = np.asarray(z_got).astype(LD)
    with np.errstate(all="ignore"):
        e_main = np.abs(g - z)
        ok_main = np.where(z == 0, g == 0, e_main <= b)
        alt = np.where(z == 0, cand, 0)
        ok_alt = uns & np.where(alt == 0, g == 0, np.abs(g - alt) <= b)
        e = np.where(ok_main, e_main, np.abs(g - alt))
        ratio = np.where((b > 0) & (g != 0), e / np.where(b > 0, b, 1), 0)
    ok = ok_main | ok_alt | ~fin
    return np.flatnonzero(~ok), float(np.max(ratio[fin & ok], initial=0.0)), uns


def g_bound(n, dtype):
    return (math.ceil(math.log2(max(n, 2))) + POW_ULP + 2) * float(np.finfo(dtype).eps)


def g_exact(z, p, alpha, dtype):
    """alpha * sum z^p in long double over z as given, with p and alpha as the device holds them"""
    T = np.dtype(dtype).type
    zl = np.asarray(z).astype(LD)
    with np.errstate(all="ignore"):
        return LD(T(alpha)) * np.sum(zl ** LD(T(p)))


# ---------------------------------------------------------------------------------------------- the table
# u of the Box kind, per entry, by its index in the block modulo len(U_CHOICES); z is the entry's z* (x / 2 where it has
# none) and uc the bound at which phi(uc) = phi(0) (z / 2 where there is none)
U_CHOICES = ("zero", "subnormal", "half", "pred", "at", "succ", "twice", "inf", "nan", "tie", "tie-", "tie+", "tie-k", "tie+k")
TIED_U = ("subnormal", "tie", "tie-", "tie+", "tie-k", "tie+k")              # bounds that make a tie on purpose
SPECIALS = ("nan", "+inf", "-inf", "+max", "-max")


@functools.lru_cache(maxsize=None)
def block(p, alpha, gamma, dt, kind):
    """One row of the table: (x, u, tags) of BLOCK_LEN entries in the working type; u is None for the Nonneg kind.  The
    edge entries come first (EDGE_LEN of them: the first is a threshold entry, the last one too), the random part after."""
    dtype = np.dtype(dt)
    T = dtype.type
    fi = np.finfo(dtype)
    eps = LD(fi.eps)
    pl, a = held(p, alpha, gamma, dtype)
    rng = np.random.default_rng([SEED, P_TABLE.index(p), int(alpha > 0), gammas_of(alpha).index(gamma), TYPES.index(dt)])
    sub = fi.smallest_subnormal
    xs, tags = [], []

    def add(v, tag):
        xs.append(LD(v)); tags.append(tag)
    if alpha > 0:
        z_t, x_t, zbar, psi = threshold(pl, a)
        add(x_t * (1 + 256 * eps), "thr+256")
        for k in K_LIST:
            for s in (+1, -1):
                if (k, s) != (256, +1) and (k, s) != (4096, -1):
                    add(x_t * (1 + s * k * eps), "thr%s%d" % ("+" if s > 0 else "-", k))
        for f in (0.1, 0.5, 0.9):
            add(psi + LD(f) * (x_t - psi), "between")
        add(-2 * x_t, "neg")
    else:
        for v in (1e-3, 1.0, 0.3, 1e6, 47.0):
            add(v, "a0")
        for v in (1e-17, 1e-16, 2e-16, 1e-9, 5e-8, 7e-8, 1e-7, 6e-9, 1e-30):
            add(v, "a0-tiny")
        add(-1.0, "neg")
    add(0.0, "+0"); add(-0.0, "-0")
    add(sub, "sub"); add(-LD(sub), "sub"); add(LD(fi.tiny) * (1 - eps), "sub")
    for v, t in zip((np.nan, np.inf, -np.inf, fi.max, -LD(fi.max)), SPECIALS):
        add(v, "special")
    if alpha > 0:
        add(x_t * (1 - 4096 * eps), "thr-4096")
    else:
        add(2.5, "a0")
    n_edge = len(xs)
    assert n_edge == EDGE_LEN
    nr = BLOCK_LEN - n_edge
    if alpha > 0:
        mag = x_t * LD(10.0) ** rng.uniform(-8, 6, nr).astype(LD)
        sign = np.where(rng.random(nr) < 0.25, -1, 1)
        rnd, rtag = list(mag * sign), ["random"] * nr
    else:
        third = nr // 3
        big = LD(10.0) ** rng.uniform(-3, 6, nr - 2 * third).astype(LD)
        neg = -(LD(10.0) ** rng.uniform(-8, 6, third).astype(LD))
        tiny = LD(10.0) ** rng.uniform(-30, -3, third).astype(LD)
        rnd = list(big) + list(neg) + list(tiny)
        rtag = ["a0"] * len(big) + ["neg"] * third + ["a0-tiny"] * third
        order = rng.permutation(nr)
        rnd, rtag = [rnd[i] for i in order], [rtag[i] for i in order]
    with np.errstate(all="ignore"):
        x = np.array(xs + rnd, LD).astype(dtype)
    x[[i for i, t in enumerate(tags) if t == "-0"]] = T(-0.0)
    tags = tags + rtag
    assert x.shape == (BLOCK_LEN,) and len(tags) == BLOCK_LEN
    u = None
    if kind == "box":
        xl = x.astype(LD)
        pos = np.isfinite(xl) & (xl > 0)
        zs = np.where(pos, xl / 2, 1)
        st = np.full(BLOCK_LEN, np.nan, LD)
        st[pos] = stationary(xl[pos], pl, a)
        kept = pos & np.isfinite(st)
        kept[kept] = _phi(st[kept], xl[kept], pl, a) < LD(0.5) * xl[kept] ** 2
        zs = np.where(kept, st, zs)
        uc = zs / 2
        if alpha > 0 and np.any(kept):
            uc[kept] = tie_bound(xl[kept], st[kept], pl, a)
        zT = zs.astype(dtype)
        ucT = uc.astype(dtype)
        with np.errstate(all="ignore"):
            by = {"zero": np.zeros(BLOCK_LEN, dtype), "subnormal": np.full(BLOCK_LEN, sub, dtype), "half": (zs / 2).astype(dtype),
                  "pred": np.nextafter(zT, T(0)), "at": zT, "succ": np.nextafter(zT, T(np.inf)), "twice": (2 * zs).astype(dtype),
                  "inf": np.full(BLOCK_LEN, np.inf, dtype), "nan": np.full(BLOCK_LEN, np.nan, dtype), "tie": ucT,
                  "tie-": np.nextafter(ucT, T(0)), "tie+": np.nextafter(ucT, T(np.inf)),
                  "tie-k": (uc * (1 - 4096 * eps)).astype(dtype), "tie+k": (uc * (1 + 4096 * eps)).astype(dtype)}
        which = np.arange(BLOCK_LEN) % len(U_CHOICES)
        u = np.empty(BLOCK_LEN, dtype)
        for j, name in enumerate(U_CHOICES):
            u[which == j] = by[name][which == j]
        u = np.where(np.isnan(u) | (u >= 0), u, T(0)).astype(dtype)
        u[np.isinf(x) | np.isnan(x)] = T(1)
        tags = [t + "|u=" + U_CHOICES[i % len(U_CHOICES)] for i, t in enumerate(tags)]
        u.setflags(write=False)
    x.setflags(write=False)
    return x, u, tuple(tags), n_edge


def layout(n):
    """indices into a block for a vector of length n: the block tiled, and the edge entries again at the very end, so that
    threshold and special entries sit at the start, across the pack boundaries of the ragged tail and in the last element"""
    idx = np.arange(n) % BLOCK_LEN
    if n > EDGE_LEN:
        idx[n - EDGE_LEN:] = np.arange(EDGE_LEN)
    return idx


@functools.lru_cache(maxsize=None)
def block_twin(p, alpha, gamma, dt, kind):
    x, u, tags, _ = block(p, alpha, gamma, dt, kind)
    pl, a = held(p, alpha, gamma, dt)
    tw = twin(x, u, pl, a)
    for v in tw:
        v.setflags(write=False)
    return tw


def oracle_prox(x, u, p, alpha, gamma, dtype):
    """the oracle's prox and value on the arguments in the working type"""
    T = np.dtype(dtype).type
    g = ref.NormLpPowerNonneg(T(p), alpha=T(alpha)) if u is None else ref.NormLpPowerBox(T(p), T(alpha), u=u)
    z = np.empty_like(x)
    with np.errstate(all="ignore"):
        gz = g.prox(z, x, T(gamma))
    return z, gz


def rows():
    return [(p, alpha, gamma) for p in P_TABLE for alpha in ALPHAS for gamma in gammas_of(alpha)]


# ---------------------------------------------------------------------------------------------- a counting copy of the loop
def counted_loop(x, p, alpha, gamma, u, rule):
    """The oracle's loop with a step count per element.  rule = "reference": |dphi| <= 1e-12 or 1000 steps alone;
    rule = "restated": the oracle's present rule.  Returns (result, steps, ended_by_tolerance); elements that never enter
    the loop have 0 steps."""
    T = x.dtype.type
    box = u is not None
    a = T(alpha) * T(gamma)
    p = T(p)
    out, steps, tol_end = np.zeros_like(x), np.zeros(x.shape, int), np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        ap = a * p
        zbar = (T(1) / (ap * (T(1) - p))) ** (T(1) / (p - T(2)))
        psi = zbar + ap * zbar ** (p - T(1))
        act = ~(x <= 0) & ~(psi >= x)
        if box:
            act &= ~(u == 0)
        if not np.any(act):
            return out, steps, tol_end
        xa = x[act]
        z = np.full_like(xa, zbar + (T(0.1) if box else T(1)))
        run, by_tol = np.ones(xa.shape, bool), np.zeros(xa.shape, bool)
        cnt = np.zeros(xa.shape, int)
        seen, prev, zprev = np.zeros(xa.shape, bool), np.zeros_like(xa), z.copy()
        for _ in range(1000):
            dphi = z - xa + ap * z ** (p - T(1))
            adphi = np.abs(dphi)
            hit = run & (adphi <= 1e-12)
            by_tol |= hit
            run &= ~hit
            if rule == "restated":
                back = run & seen & (adphi >= prev)
                z = np.where(back, zprev, z)
                run &= ~back
            if not np.any(run):
                break
            seen |= run & (dphi > 0)
            upd = run & seen
            prev = np.where(upd, adphi, prev)
            zprev = np.where(upd, z, zprev)
            ddphi = T(1) + ap * (p - T(1)) * z ** (p - T(2))
            zn = np.where(run, z - dphi / ddphi, z)
            cnt += run
            if rule == "restated":
                run &= ~(zn == z) & ~(zn != zn)
            z = zn
        phi0 = T(0.5) * (xa * xa)
        phiz = T(0.5) * (z - xa) ** 2 + a * z ** p
        res = np.where(phi0 <= phiz, T(0), z)
        if box:
            ua = u[act]
            phiu = T(0.5) * (ua - xa) ** 2 + a * ua ** p
            over = (res != 0) & (z > ua)
            res = np.where(over, np.where(phiu < phi0, ua, T(0)), res)
    out[act], steps[act], tol_end[act] = res, cnt, by_tol
    return out, steps, tol_end


def same_bits(a, b):
    return bool(np.all((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- the proofs
def test_threshold_closed_form_is_a_tie():
    """phi(z_t) = phi(0) and phi'(z_t) = 0 at x = x_t, to the rounding of long double"""
    for p in P_TABLE:
        for gamma in GAMMAS:
            pl, a = held(p, 0.8, gamma, np.float64)
            z_t, x_t, zbar, psi = threshold(pl, a)
            assert zbar < z_t and psi < x_t
            assert abs(_phi(z_t, x_t, pl, a) - LD(0.5) * x_t * x_t) <= 8 * np.finfo(LD).eps * x_t * x_t
            assert abs(_dphi(z_t, x_t, pl, a)) <= 8 * np.finfo(LD).eps * x_t


def test_twin_against_mpmath():
    """the twin's stationary point and decision against a 40-digit bisection, on a sample of every row"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    worst = 0.0
    for p, alpha, gamma in rows():
        if alpha == 0:
            continue
        x, _, tags, _ = block(p, alpha, gamma, "float64", "nonneg")
        pl, a = held(p, alpha, gamma, np.float64)
        z, cand, margin = block_twin(p, alpha, gamma, "float64", "nonneg")
        pm, am = mp.mpf(float(pl)), mp.mpf(float(a))
        picks = [i for i, t in enumerate(tags) if t.startswith("thr") or t == "between"][:8] + \
                [i for i, t in enumerate(tags) if t == "random" and cand[i] > 0][:6]
        for i in picks:
            xm = mp.mpf(float(x[i]))
            d = lambda v: v - xm + am * pm * v ** (pm - 1)
            lo, hi = (am * pm * (1 - pm)) ** (1 / (2 - pm)), xm
            if d(lo) >= 0:
                assert cand[i] == 0, (p, gamma, tags[i])
                continue
            for _ in range(140):
                mid = (lo + hi) / 2
                if d(mid) > 0:
                    hi = mid
                else:
                    lo = mid
            zm = (lo + hi) / 2
            # (phi' is a difference of terms of size x evaluated to a few long-double ulps, and phi'' > 1/2: 16 eps x)
            err = abs(mp.mpf(float(cand[i])) + mp.mpf(float(cand[i] - LD(float(cand[i])))) - zm) / xm
            worst = max(worst, float(err))
            assert err <= 16 * float(np.finfo(LD).eps), (p, gamma, tags[i], float(err))
            mm = mp.mpf("0.5") * xm * xm - (am * zm ** pm + mp.mpf("0.5") * (zm - xm) ** 2)
            if abs(mm) > 1e-17 * xm * xm:
                assert (z[i] != 0) == (mm > 0), (p, gamma, tags[i])
    print("twin against mpmath: worst |z* - z_mp| / x = %.2e" % worst)


def _nonspecial(tags):
    return np.array(["special" not in t for t in tags])


def test_caps_on_unsettled_entries_and_settled_threshold_rows():
    """On the twin alone: (1) unsettled entries are at most 0.1 % of the random part of every row (for the Box kind: of
    the random part whose u is not one of TIED_U, the bounds that make a tie on purpose); (2) the threshold rows with
    k >= 256 (1024 at p = 0.99: k_settled) are settled and those with k <= 8 are unsettled, for every p, gamma and type."""
    shares = {}
    for dt in TYPES:
        for kind in KINDS:
            worst, tot_u, tot = 0.0, 0, 0
            for p, alpha, gamma in rows():
                x, u, tags, _ = block(p, alpha, gamma, dt, kind)
                z, cand, margin = block_twin(p, alpha, gamma, dt, kind)
                uns = unsettled(x, margin, dt)
                rnd = np.array([t.split("|")[0] in ("random", "a0", "neg") and t.split("=")[-1] not in TIED_U for t in tags])
                share = float(np.sum(uns & rnd)) / float(np.sum(rnd))
                worst, tot_u, tot = max(worst, share), tot_u + int(np.sum(uns & rnd)), tot + int(np.sum(rnd))
                assert share <= 1e-3, (dt, kind, p, alpha, gamma, [tags[i] for i in np.flatnonzero(uns & rnd)])
                if alpha > 0 and kind == "nonneg":
                    assert k_settled(p) == (1024 if p == 0.99 else 256)
                    for i, t in enumerate(tags):
                        if t.startswith("thr"):
                            k = int(t[4:])
                            if k >= k_settled(p):
                                assert not uns[i], (dt, p, gamma, t)
                                assert (z[i] != 0) == (t[3] == "+"), (dt, p, gamma, t)
                            if k <= 8:
                                assert uns[i], (dt, p, gamma, t)
            shares[(dt, kind)] = (tot_u, tot, worst)
    print("unsettled shares of the random part (entries, of, worst row):", shares)


def test_oracle_meets_the_bounds_over_the_table():
    """The oracle through judge() and the g bound in both types and kinds over every row: every GPU expectation is
    reachable.  Prints the largest error / bound per type."""
    for dt in TYPES:
        worst, worst_g = 0.0, 0.0
        for kind in KINDS:
            for p, alpha, gamma in rows():
                x, u, tags, _ = block(p, alpha, gamma, dt, kind)
                tw = block_twin(p, alpha, gamma, dt, kind)
                z, gz = oracle_prox(x, u, p, alpha, gamma, dt)
                fin = judged(x, dt)
                if alpha == 0:
                    # the tiny-argument corner: NaN where the right value is min(x, u); elsewhere the clamp within the bound
                    bad, ratio, uns = judge(z, x, tw, dt, hold=(x >= 1e-3) | (x <= 0))
                else:
                    bad, ratio, uns = judge(z, x, tw, dt)
                    assert not np.any(np.isnan(z[fin])), (dt, kind, p, gamma)
                assert bad.size == 0, (dt, kind, p, alpha, gamma, [(tags[i], x[i], None if u is None else u[i], z[i], tw[0][i]) for i in bad[:5]])
                worst = max(worst, ratio)
                if alpha > 0:
                    m = fin & np.isfinite(z)
                    ex = g_exact(z[m], p, alpha, dt)
                    zz, gg = oracle_prox(x[m], None if u is None else u[m], p, alpha, gamma, dt)
                    assert same_bits(zz, z[m])
                    assert abs(LD(gg) - ex) <= g_bound(int(np.sum(m)), dt) * ex, (dt, kind, p, gamma, gg, ex)
                    if ex > 0:
                        worst_g = max(worst_g, float(abs(LD(gg) - ex) / ex) / g_bound(int(np.sum(m)), dt))
        print("oracle %s: largest |z - z*| / bound %.3f, largest g error / bound %.3f" % (dt, worst, worst_g))
        assert worst <= 1.0


def test_alpha_zero_is_the_clamp_and_the_tiny_corner_is_nan():
    """alpha = 0 on the oracle: the prox is min(x, u) within eps max(z0, x) (the rounding of z0 - x and that of the step
    z0 - (z0 - x); u itself where it binds); 0 for x <= 0; and the tiny-argument corner, where z0 - x rounds to z0, returns
    NaN where the right value is x.  Prints the share of entries that are the clamp bit for bit."""
    for dt in TYPES:
        T = np.dtype(dt).type
        eps = float(np.finfo(dt).eps)
        exact = [0, 0]
        for kind in KINDS:
            for p in P_TABLE:
                x, u, tags, _ = block(p, 0.0, 0.37, dt, kind)
                z, _ = oracle_prox(x, u, p, 0.0, 0.37, dt)
                xl = x.astype(np.float64)
                ub = np.full(x.shape, np.inf) if u is None else np.where(np.isnan(u), np.inf, u).astype(np.float64)
                # (a bound u > 0 below eps x cannot win phi(u) < phi(0) in the working type: such entries are unsettled)
                big = judged(x, dt) & (xl >= 1e-3) & ((ub == 0) | (ub >= eps * xl))
                clamp = np.minimum(xl, ub)
                z0 = 1.0 if kind == "nonneg" else 0.1
                assert np.all(np.abs(z[big] - clamp[big]) <= eps * np.maximum(z0, xl[big])), (dt, kind, p)
                exact[0] += int(np.sum(z[big] == clamp[big])); exact[1] += int(np.sum(big))
                assert np.all(z[np.isfinite(xl) & (xl <= 0)] == 0)
                tiny = np.isfinite(xl) & (xl > 0) & (xl < (0.03 if kind == "box" else 0.25) * eps) & (ub > 0)
                assert np.sum(tiny) >= 20 and np.all(np.isnan(z[tiny])), (dt, kind, p, x[tiny][~np.isnan(z[tiny])][:4])
        print("alpha = 0, %s: %d of %d entries with x >= 1e-3 are min(x, u) bit for bit" % (dt, exact[0], exact[1]))


# the largest number of Newton steps the restated loop takes over the table, measured on the oracle; asserted with a
# margin of 2 x (condition (c)).  The reference's rule takes 1000 on the entries counted in NEXT.md.
MAX_STEPS_MEASURED = {"float64": 8, "float32": 9}


def test_restated_stopping_rule_conditions():
    """Conditions (a)-(d) on the rule that ends the Newton loop once rounding has taken over, over the whole table, with
    the counting copy of the loop: (0) the copy under "restated" is the oracle, bit for bit; (a) fp64 entries that the
    reference's loop ends by its 1e-12 test keep their bits; (b) no entry leaves the bound on z (that is
    test_oracle_meets_the_bounds_over_the_table, which runs the restated oracle); (c) the step count is bounded; (d) the
    supports of settled entries do not change."""
    for dt in TYPES:
        most_new, full_old, entered, changed, by_tol = 0, 0, 0, 0, 0
        for kind in KINDS:
            for p, alpha, gamma in rows():
                x, u, tags, _ = block(p, alpha, gamma, dt, kind)
                tw = block_twin(p, alpha, gamma, dt, kind)
                z_new, s_new, _ = counted_loop(x, p, alpha, gamma, u, "restated")
                z_old, s_old, t_old = counted_loop(x, p, alpha, gamma, u, "reference")
                z_orc, _ = oracle_prox(x, u, p, alpha, gamma, dt)
                assert same_bits(z_new, z_orc), (dt, kind, p, alpha, gamma)
                fin = judged(x, dt)
                if dt == "float64":
                    assert same_bits(z_new[t_old & fin], z_old[t_old & fin]), (dt, kind, p, alpha, gamma)          # (a)
                changed += int(np.sum((z_new != z_old)[t_old & fin]))
                by_tol += int(np.sum(t_old & fin))
                most_new = max(most_new, int(np.max(s_new[fin])))                                                 # (c)
                full_old += int(np.sum(s_old[fin] >= 1000))
                entered += int(np.sum(s_old[fin] > 0))
                settled = fin & ~unsettled(x, tw[2], dt) & ~np.isnan(z_old) & ~np.isnan(z_new)
                assert np.array_equal((z_new != 0)[settled], (z_old != 0)[settled]), (dt, kind, p, alpha, gamma)  # (d)
        print("%s: restated rule takes at most %d steps; the reference's rule runs all 1000 on %d of %d entries that enter "
              "the loop; %d of its %d tolerance-ended entries change bits" % (dt, most_new, full_old, entered, changed, by_tol))
        assert most_new <= 2 * MAX_STEPS_MEASURED[dt]


# ---------------------------------------------------------------------------------------------- short trajectories
TRAJ_N, TRAJ_STATES, TRAJ_P = 1031, 20, (0.1, 0.9)


class WatchedG:
    """the oracle's g with a watch on every prox call: `hit` is set once an argument has an entry that is unsettled by
    the rule above, i.e. once a device that is right may take the other branch and the iterates part for good"""

    def __init__(self, g, p, alpha, u, dt):
        self.g, self.p, self.alpha, self.u, self.dt, self.hit, self.calls = g, p, alpha, u, dt, False, 0

    def __call__(self, x):
        return self.g(x)

    def prox(self, z, x, gamma):
        pl, a = held(self.p, self.alpha, gamma, self.dt)
        tw = twin(x, self.u, pl, a)
        self.calls += 1
        self.hit |= bool(np.any(unsettled(x, tw[2], self.dt) & judged(x, self.dt)))
        with np.errstate(all="ignore"):
            return self.g.prox(z, x, gamma)


def trajectory_problem(m, p, kind, dt):
    """the cfg-2 family (DiagQuadratic f, c = Identity, D a box) with an Lp g, for the module m (the device's classes or the
    oracle's); also (mu, y, x0, u)"""
    import bazinga_jl_amd as bz
    dtype = np.dtype(dt)
    T = dtype.type
    n = TRAJ_N
    d = bz.synth.l1_quadratic(n, dtype=dtype)
    u = np.where(np.arange(n) % 5 == 0, 0.0, 0.9).astype(dtype) if kind == "box" else None
    num = (lambda v: T(v)) if m is ref else float
    g = m.NormLpPowerNonneg(num(p), alpha=num(0.8)) if kind == "nonneg" else m.NormLpPowerBox(num(p), num(0.8), u=u)
    D = m.ClosedSet(m.IndBox(num(d["lo"]), num(d["hi"])))
    rng = np.random.default_rng(1031)
    mu, y, x0 = np.full(n, 0.1, dtype), rng.standard_normal(n).astype(dtype), np.zeros(n, dtype)
    return (m.DiagQuadratic(d["q"], d["b"]), g, m.IdentityFunction(), D), mu, y, x0, u


@functools.lru_cache(maxsize=None)
def oracle_trajectory(p, kind, dt):
    """TRAJ_STATES PANOCplus states of the oracle: [(x, z, gamma, sensitivity)], and how many of them come before the
    first prox call with an unsettled entry (those are compared with the device).  The sensitivity is the distance to a
    second run of the oracle with long-double sums, as in tests/test_gpu_parity.py."""
    from tests.test_gpu_parity import LongDoubleReducer, _err
    orc, mu, y, x0, u = trajectory_problem(ref, p, kind, dt)
    watch = WatchedG(orc[1], p, 0.8, u, dt)
    its, sts = [], []
    for red, g in ((None, watch), (LongDoubleReducer(), orc[1])):
        ref.set_reducer(red)
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(g), x0, minimum_gamma=1e-7)
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    states, compared, env = [], None, 0.0
    for k in range(TRAJ_STATES):
        if watch.hit and compared is None:
            compared = k
        env = max(env, _err(sts[1].x, sts[0].x), _err(sts[1].z, sts[0].z))
        states.append((sts[0].x.copy(), sts[0].z.copy(), float(sts[0].gamma), env))
        if k + 1 < TRAJ_STATES:
            sts[0] = its[0].step(sts[0])
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    return states, TRAJ_STATES if compared is None else compared, watch.calls


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", TRAJ_P)
def test_trajectories_have_ten_compared_states(p, kind, dt):
    """on the oracle alone: at least 10 of the 20 states of every run come before the first unsettled entry"""
    states, compared, calls = oracle_trajectory(p, kind, dt)
    supp = [int(np.count_nonzero(s[1])) for s in states]
    print("trajectory p=%.1f %s %s: %d states compared, %d prox calls, support %d -> %d, gamma %.3g -> %.3g"
          % (p, kind, dt, compared, calls, supp[0], supp[-1], states[0][2], states[-1][2]))
    assert len(states) == TRAJ_STATES and compared >= 10
    assert max(supp) > 0
