"""Synthetic inputs for the BASELINE configs.

Language-independent uniform stream so C/HIP/Python/Julia produce identical bits:

    u_k(i) = (splitmix64(seed + k*2^60 + i) >> 11) * 2^-53      seed = 20241004

(the top 53 bits, so the conversion to double is exact in every language).
"""
from __future__ import annotations

import numpy as np

SEED = 20241004
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x: np.ndarray) -> np.ndarray:
    """One splitmix64 output per uint64 input (vectorised, wrap-around arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform(k: int, n: int, start: int = 0, seed: int = SEED) -> np.ndarray:
    """u_k(start .. start+n-1) as float64 in [0,1)."""
    with np.errstate(over="ignore"):
        base = np.uint64(seed) + (np.uint64(k) << np.uint64(60)) + np.uint64(start)
        idx = base + np.arange(n, dtype=np.uint64)
    z = splitmix64(idx)
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def l1_quadratic(n: int, start: int = 0, dtype=np.float64):
    """cfg 2 / cfg 5 data for elements [start, start+n): q_i = 0.1 + 9.9 u1, b_i = 10(2 u2 - 1).
    f(x)=sum x(0.5 q x - b), g = 2.5||x||_1, c = I, D = Box[-1,1]."""
    q = (0.1 + 9.9 * uniform(1, n, start)).astype(dtype)
    b = (10.0 * (2.0 * uniform(2, n, start) - 1.0)).astype(dtype)
    return {"q": q, "b": b, "lam": 2.5, "lo": -1.0, "hi": 1.0}


def obstacle_grid(nx: int = 2048, ny: int | None = None, dtype=np.float64, load: float = 1.0):
    """cfg 3: 5-pt Laplacian QP on an nx-by-ny grid, b = load*h^2 (SURVEY: load = +1; load = -1
    pushes the membrane onto the obstacle so the constraint is active), obstacle
    psi_ij = 0.05 - 0.5((i h - .5)^2 + (j h - .5)^2), h = 1/(nx+1), i,j = 1..n;
    D = Box[psi, +inf), x0 = max(0, psi)."""
    ny = nx if ny is None else ny
    h = 1.0 / (nx + 1)
    i = (np.arange(1, nx + 1) * h - 0.5) ** 2
    j = (np.arange(1, ny + 1) * (1.0 / (ny + 1)) - 0.5) ** 2
    psi = (0.05 - 0.5 * (i[:, None] + j[None, :])).reshape(-1).astype(dtype)
    b = np.full(nx * ny, load * h * h, dtype=dtype)
    return {"nx": nx, "ny": ny, "b": b, "psi": psi, "x0": np.maximum(0, psi).astype(dtype)}


def basis_pursuit(ny: int = 8192, n: int = 65536, dtype=np.float32, density: float = 0.01):
    """cfg 4: A_ij = (2 u3 - 1)/sqrt(ny) row-major ny-by-n, xtrue density-sparse +-1, b = A xtrue."""
    A = np.empty((ny, n), dtype=dtype)
    rows = max(1, (1 << 24) // n)
    s = 1.0 / np.sqrt(ny)
    for r0 in range(0, ny, rows):
        r1 = min(ny, r0 + rows)
        A[r0:r1] = ((2.0 * uniform(3, (r1 - r0) * n, r0 * n) - 1.0) * s).reshape(r1 - r0, n).astype(dtype)
    u = uniform(4, n)
    sgn = np.where(uniform(5, n) < 0.5, -1.0, 1.0)
    xtrue = np.where(u < density, sgn, 0.0).astype(dtype)
    b = (A.astype(np.float64) @ xtrue.astype(np.float64)).astype(dtype)
    return {"A": A, "b": b, "xtrue": xtrue}


def obstacle_1d(N: int, dtype=np.float64):
    """The constraint map of the one-dimensional obstacle problem, c(x) = x1 + T x2 - x3 on x = [x1; x2; x3] with
    T = tridiag(-1, 2, -1): the CSR of [I, T, -I] (ny = N, n = 3N, at most five entries per row), b = 0, D = ZeroSet
    (x = 0 is feasible).  With it a DiagQuadratic f: q_i = 0.5 + u1, b_i = 2 u2 - 1."""
    i = np.arange(N, dtype=np.int64)
    cols = np.stack([i, N + i - 1, N + i, N + i + 1, 2 * N + i], axis=1)
    vals = np.tile(np.array([1.0, -1.0, 2.0, -1.0, -1.0]), (N, 1))
    keep = np.ones((N, 5), bool)
    keep[0, 1] = False
    keep[N - 1, 3] = False
    indptr = np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.int64)
    n = 3 * N
    return {"indptr": indptr, "indices": cols[keep].astype(np.int32), "data": vals[keep].astype(dtype),
            "b": np.zeros(N, dtype), "n": n, "ny": N,
            "q": (0.5 + uniform(1, n)).astype(dtype), "fb": (2.0 * uniform(2, n) - 1.0).astype(dtype)}


def budget_bands(n: int, m: int, dtype=np.float64):
    """A budget row beside band rows (ny = m + 1): row 0 is sum_i x_i = 1 (n entries, D_0 = {0} with b_0 = 1); row k >= 1
    has three consecutive entries a = 2 u3 - 1 starting at column ((k - 1)(n - 4)) div m and one entry in column n - 1,
    which every band row shares, with b_k = 0 and D_k = [lo_k, hi_k] drawn around the row's value at a point xfeas of
    the simplex: the constraints are consistent.  With it g = IndBox(0, 1) and a DiagQuadratic f: q_i = 0.5 + u1,
    b_i = 2 u2 - 1."""
    if n < 5 or m < 1:
        raise ValueError("budget_bands needs n >= 5 and m >= 1")
    k = np.arange(m, dtype=np.int64)
    start = (k * (n - 4)) // m
    bcols = np.stack([start, start + 1, start + 2, np.full(m, n - 1, np.int64)], axis=1)
    bvals = (2.0 * uniform(3, 4 * m) - 1.0).reshape(m, 4)
    indptr = np.concatenate(([0], n + 4 * np.arange(m + 1, dtype=np.int64)))
    indices = np.concatenate((np.arange(n, dtype=np.int64), bcols.reshape(-1))).astype(np.int32)
    data = np.concatenate((np.ones(n), bvals.reshape(-1))).astype(dtype)
    xfeas = uniform(4, n)
    xfeas /= xfeas.sum()
    at = (data[n:].astype(np.float64).reshape(m, 4) * xfeas[bcols]).sum(axis=1)      # the band rows at xfeas
    lo = np.concatenate(([0.0], at - 0.1 * uniform(5, m))).astype(dtype)
    hi = np.concatenate(([0.0], at + 0.1 * uniform(6, m))).astype(dtype)
    b = np.zeros(m + 1, dtype)
    b[0] = 1
    return {"indptr": indptr, "indices": indices, "data": data, "b": b, "n": n, "ny": m + 1, "lo": lo, "hi": hi,
            "xfeas": xfeas.astype(dtype), "q": (0.5 + uniform(1, n)).astype(dtype),
            "fb": (2.0 * uniform(2, n) - 1.0).astype(dtype)}


def laplacian_2d(nx: int, ny: int, dtype=np.float64):
    """The matrix of Stencil5ptQuadratic as CSR: the 5-point Laplacian (4, -1, -1, -1, -1) on an nx-by-ny grid (row-major,
    index = i*ny + j) with the homogeneous Dirichlet halo dropped.  Entry order per row: centre, west, east, north, south."""
    i, j = np.divmod(np.arange(nx * ny, dtype=np.int64), ny)
    c = i * ny + j
    cols = np.stack([c, c - 1, c + 1, c - ny, c + ny], axis=1)
    keep = np.stack([np.ones(nx * ny, bool), j > 0, j < ny - 1, i > 0, i < nx - 1], axis=1)
    vals = np.tile(np.array([4.0, -1.0, -1.0, -1.0, -1.0]), (nx * ny, 1))
    indptr = np.concatenate(([0], np.cumsum(keep.sum(axis=1)))).astype(np.int64)
    return {"indptr": indptr, "indices": cols[keep].astype(np.int32), "data": vals[keep].astype(dtype), "n": nx * ny}


def sparse_qp(n: int, m: int, seed: int = SEED, dtype=np.float64):
    """A sparse QP: min 0.5 x'Qx + q'x over the constraints of budget_bands(n, m), with g = IndBox(0, 1).  Q is symmetric
    and strictly diagonally dominant (positive definite) with about seven entries per row: the off-diagonals at the
    distances 1, 7 and 31, w_k(i) = -(0.1 + 0.4 u_k) between i and i + d_k, and the diagonal 0.5 + u4 plus the row's
    absolute off-diagonal sum.  q_i = 2 u5 - 1.  The entries of a row are stored by ascending column."""
    if n < 32:
        raise ValueError("sparse_qp needs n >= 32")
    i = np.arange(n, dtype=np.int64)
    rows, cols, vals = [], [], []
    offsum = np.zeros(n)
    for k, dist in enumerate((1, 7, 31)):
        w = -(0.1 + 0.4 * uniform(1 + k, n - dist, seed=seed))
        rows += [i[:-dist], i[dist:]]
        cols += [i[dist:], i[:-dist]]
        vals += [w, w]
        offsum[:-dist] += -w
        offsum[dist:] += -w
    rows.append(i); cols.append(i); vals.append(0.5 + uniform(4, n, seed=seed) + offsum)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)
    out = budget_bands(n, m, dtype)
    out.update({"Q_indptr": indptr, "Q_indices": cols[order].astype(np.int32), "Q_data": vals[order].astype(dtype),
                "fq": (2.0 * uniform(5, n, seed=seed) - 1.0).astype(dtype)})
    return out


def _sparse_rows(m: int, n: int, k: int, dtype, seed: int):
    """the matrix and the planted x* that sparse_lasso describes: (cols[m][k], data[m k], x* in float64, A x* in float64)"""
    lo = (np.arange(k + 1, dtype=np.int64) * n) // k
    width = np.diff(lo)
    inside = np.floor(uniform(1, m * k, seed=seed).reshape(m, k) * width).astype(np.int64)
    shift = np.floor(uniform(2, m, seed=seed) * n).astype(np.int64)
    cols = (lo[:-1] + inside + shift[:, None]) % n
    order = np.argsort(uniform(3, m * k, seed=seed).reshape(m, k), axis=1, kind="stable")
    cols = np.take_along_axis(cols, order, axis=1)
    data = ((2.0 * uniform(4, m * k, seed=seed) - 1.0) / np.sqrt(k)).astype(dtype)
    nz = max(1, n // 20)
    support = np.argsort(uniform(5, n, seed=seed), kind="stable")[:nz]
    xstar = np.zeros(n)
    xstar[support] = (1.0 + uniform(6, nz, seed=seed)) * np.where(uniform(7, nz, seed=seed) < 0.5, -1.0, 1.0)
    return cols, data, xstar, (data.astype(np.float64).reshape(m, k) * xstar[cols]).sum(axis=1)


def sparse_lasso(m: int, n: int, k: int = 5, dtype=np.float64, seed: int = SEED):
    """A sparse Lasso: min 0.5||A x - b||^2 + lam ||x||_1 with A m-by-n in CSR, k entries per row at distinct random columns:
    [0, n) is cut into k strata [j n div k, (j + 1) n div k), row i takes the column floor(u1 w_j) of stratum j, shifted by
    the row's offset floor(u2 n) modulo n, and stores its k entries in the order of the keys u3 (the columns are unsorted).
    a_ij = (2 u4 - 1) / sqrt(k).  A planted x* with max(1, n div 20) entries 1 + u6 of random sign (u7) at the columns of
    the smallest keys u5; b = A x* + 0.01 (2 u8 - 1)."""
    if not 1 <= k <= n or m < 1:
        raise ValueError("sparse_lasso needs m >= 1 and 1 <= k <= n")
    cols, data, xstar, Axstar = _sparse_rows(m, n, k, dtype, seed)
    b = Axstar + 0.01 * (2.0 * uniform(8, m, seed=seed) - 1.0)
    return {"indptr": k * np.arange(m + 1, dtype=np.int64), "indices": cols.reshape(-1).astype(np.int32), "data": data,
            "b": b.astype(dtype), "m": m, "n": n, "xstar": xstar.astype(dtype)}


def sparse_logistic(m: int, n: int, k: int = 5, dtype=np.float64, seed: int = SEED):
    """Sparse logistic regression: min sum_i log(1 + exp(-b_i a_i'x)) + lam ||x||_1 with the matrix and the planted x* of
    sparse_lasso(m, n, k, dtype, seed) and the labels b_i = +1 if (A x*)_i + 0.1 (2 u9 - 1) >= 0 else -1 (a tenth of the
    margins' scale in noise: a few labels near the boundary are flipped, so the classes are not separable by x*)."""
    if not 1 <= k <= n or m < 1:
        raise ValueError("sparse_logistic needs m >= 1 and 1 <= k <= n")
    cols, data, xstar, Axstar = _sparse_rows(m, n, k, dtype, seed)
    labels = np.where(Axstar + 0.1 * (2.0 * uniform(9, m, seed=seed) - 1.0) >= 0, 1.0, -1.0)
    return {"indptr": k * np.arange(m + 1, dtype=np.int64), "indices": cols.reshape(-1).astype(np.int32), "data": data,
            "labels": labels.astype(dtype), "m": m, "n": n, "xstar": xstar.astype(dtype)}


GLM_LOSSES = ("least_squares", "logistic", "huber", "squared_hinge", "poisson")


def sparse_glm(m: int, n: int, k: int = 5, loss: str = "huber", dtype=np.float64, seed: int = SEED):
    """A sparse GLM: min sum_i w_i l(b_i, a_i'x) + lam ||x||_1 with the matrix and the planted x* of sparse_lasso(m, n, k, dtype,
    seed) and b by the loss.  least_squares: sparse_lasso's b = A x* + 0.01 (2 u8 - 1).  huber (delta = 1): the same with a
    gross outlier in every 16th row, b_i += 10 (2 u10 - 1) + (5 or -5 by the sign of that draw) at i = 15, 31, ...  logistic and
    squared_hinge: sparse_logistic's labels.  poisson: the margins scaled into [-2, 2], t~ = 2 A x* / max|A x*| (the planted
    vector returned is scaled with them), and the counts by inverse CDF at the rate exp(t~_i): the smallest c with
    P(Poisson(rate) <= c) >= u9.  `delta` is 1 for huber and None otherwise."""
    if loss not in GLM_LOSSES:
        raise ValueError(f"loss must be one of {GLM_LOSSES}")
    if not 1 <= k <= n or m < 1:
        raise ValueError("sparse_glm needs m >= 1 and 1 <= k <= n")
    cols, data, xstar, Axstar = _sparse_rows(m, n, k, dtype, seed)
    delta = None
    if loss in ("logistic", "squared_hinge"):
        b = np.where(Axstar + 0.1 * (2.0 * uniform(9, m, seed=seed) - 1.0) >= 0, 1.0, -1.0)
    elif loss == "poisson":
        top = float(np.max(np.abs(Axstar)))
        s = 2.0 / top if top > 0 else 1.0
        xstar, rate = s * xstar, np.exp(s * Axstar)
        u = uniform(9, m, seed=seed)
        b = np.zeros(m)
        pmf = np.exp(-rate)
        cdf = pmf.copy()
        for c in range(1, 48):                       # (rate <= e^2: the tail beyond 47 is below 2^-53)
            b[cdf < u] = c
            pmf = pmf * rate / c
            cdf += pmf
    else:
        b = Axstar + 0.01 * (2.0 * uniform(8, m, seed=seed) - 1.0)
        if loss == "huber":
            delta = 1.0
            out = 2.0 * uniform(10, m, seed=seed) - 1.0
            rows = np.arange(15, m, 16)
            b[rows] += 10.0 * out[rows] + np.where(out[rows] >= 0, 5.0, -5.0)
    return {"indptr": k * np.arange(m + 1, dtype=np.int64), "indices": cols.reshape(-1).astype(np.int32), "data": data,
            "b": b.astype(dtype), "m": m, "n": n, "xstar": xstar.astype(dtype), "loss": loss, "delta": delta}


def sparse_multinomial(m: int, n_f: int, K: int, k: int = 5, dtype=np.float64, seed: int = SEED):
    """Sparse multinomial (softmax) regression: min sum_i (logsumexp_c(t_ic) - t_{i,b_i}) + lam ||X||_1, T = A X, with the
    matrix of sparse_lasso(m, n_f, k, dtype, seed) and a planted X* (n_f x K, row-major): its rows at the max(1, n_f div 20)
    columns of the smallest keys u5, every entry there 2 (1 + u6) of random sign (u7), drawn for the K classes of a row in a
    run.  The labels are drawn from the softmax of A X* by inverse CDF: b_i is the first class c whose cumulated probability
    reaches u9 (K - 1 if rounding leaves none).  `xstar` is the flat vector X*.reshape(-1)."""
    if not 2 <= K <= 64:
        raise ValueError("sparse_multinomial needs 2 <= K <= 64")
    if not 1 <= k <= n_f or m < 1:
        raise ValueError("sparse_multinomial needs m >= 1 and 1 <= k <= n_f")
    cols, data, _, _ = _sparse_rows(m, n_f, k, dtype, seed)
    nz = max(1, n_f // 20)
    support = np.argsort(uniform(5, n_f, seed=seed), kind="stable")[:nz]
    X = np.zeros((n_f, K))
    X[support] = (2.0 * (1.0 + uniform(6, nz * K, seed=seed)) * np.where(uniform(7, nz * K, seed=seed) < 0.5, -1.0, 1.0)).reshape(nz, K)
    t = (data.astype(np.float64).reshape(m, k, 1) * X[cols]).sum(axis=1)
    p = np.exp(t - t.max(axis=1, keepdims=True))
    cdf = np.cumsum(p / p.sum(axis=1, keepdims=True), axis=1)
    labels = np.minimum((cdf < uniform(9, m, seed=seed)[:, None]).sum(axis=1), K - 1)
    return {"indptr": k * np.arange(m + 1, dtype=np.int64), "indices": cols.reshape(-1).astype(np.int32), "data": data,
            "labels": labels.astype(dtype), "m": m, "n_f": n_f, "K": K, "n": n_f * K, "xstar": X.reshape(-1).astype(dtype)}


def sparse_multiresponse(m: int, n_f: int, K: int, per_row: int = 5, dtype=np.float64, loss: str = "least_squares", seed: int = SEED):
    """Sparse multi-response regression / multi-label classification: min sum_i sum_k l(B_ik, t_ik) + g(X), T = A X, with the
    matrix of sparse_multinomial(m, n_f, K, per_row, dtype, seed) — sparse_lasso's — and a ROW-sparse planted X* (n_f x K,
    row-major): max(1, n_f div 10) features, those of the smallest keys u5, are active in all K responses, every entry there
    (1 + u6) of random sign (u7), drawn for the K responses of a row in a run; every other row of X* is zero.  With T* = A X*:
    least_squares and huber (delta = 1): B = T* + 0.01 (2 u8 - 1) ; logistic and squared_hinge: B_ik = +1 if
    T*_ik + 0.1 (2 u9 - 1) >= 0 else -1 ; poisson: the margins scaled into [-2, 2] (X* with them) and the counts by inverse CDF at
    the rate exp(t~_ik), as sparse_glm draws them.  `B` is (m, K); `xstar` is the flat vector X*.reshape(-1)."""
    if loss not in GLM_LOSSES:
        raise ValueError(f"loss must be one of {GLM_LOSSES}")
    if not 2 <= K <= 64:
        raise ValueError("sparse_multiresponse needs 2 <= K <= 64")
    if not 1 <= per_row <= n_f or m < 1:
        raise ValueError("sparse_multiresponse needs m >= 1 and 1 <= per_row <= n_f")
    cols, data, _, _ = _sparse_rows(m, n_f, per_row, dtype, seed)
    nz = max(1, n_f // 10)
    support = np.argsort(uniform(5, n_f, seed=seed), kind="stable")[:nz]
    X = np.zeros((n_f, K))
    X[support] = ((1.0 + uniform(6, nz * K, seed=seed)) * np.where(uniform(7, nz * K, seed=seed) < 0.5, -1.0, 1.0)).reshape(nz, K)
    t = (data.astype(np.float64).reshape(m, per_row, 1) * X[cols]).sum(axis=1)
    delta = None
    if loss in ("logistic", "squared_hinge"):
        B = np.where(t + 0.1 * (2.0 * uniform(9, m * K, seed=seed).reshape(m, K) - 1.0) >= 0, 1.0, -1.0)
    elif loss == "poisson":
        top = float(np.max(np.abs(t)))
        s = 2.0 / top if top > 0 else 1.0
        X, rate = s * X, np.exp(s * t)
        u = uniform(9, m * K, seed=seed).reshape(m, K)
        B = np.zeros((m, K))
        pmf = np.exp(-rate)
        cdf = pmf.copy()
        for c in range(1, 48):                       # (rate <= e^2: the tail beyond 47 is below 2^-53)
            B[cdf < u] = c
            pmf = pmf * rate / c
            cdf += pmf
    else:
        B = t + 0.01 * (2.0 * uniform(8, m * K, seed=seed).reshape(m, K) - 1.0)
        delta = 1.0 if loss == "huber" else None
    return {"indptr": per_row * np.arange(m + 1, dtype=np.int64), "indices": cols.reshape(-1).astype(np.int32), "data": data,
            "B": np.ascontiguousarray(B.astype(dtype)), "m": m, "n_f": n_f, "K": K, "n": n_f * K, "xstar": X.reshape(-1).astype(dtype),
            "loss": loss, "delta": delta}


def portfolio(n: int, dtype=np.float64, rank: int | None = None):
    """A stand-in for the absent demo/portfolio_data (demo/portfolio.jl:70-91: Q, rho, mu, ub), from the uniform stream:

        Q  = F F' + diag(d), F n-by-r with F_ij = 0.2 (2 u1 - 1) (r = max(1, n div 10)), d_i = 0.01 + 0.04 u2
             (symmetric positive definite: a low-rank factor model plus specific risk);
        mu = 0.1 u3 in [0, 0.1], the expected returns;
        ub = (2 + 6 u4)/n, so that sum(ub) >= 2 and the budget sum(x) = 1 fits under the bounds;
        rho a quarter of the way from the return of xfeas = ub/sum(ub) to the best return the set allows (the greedy
            fill of the largest mu_i up to ub_i): {x : sum(x) = 1, mu'x >= rho, 0 <= x <= ub} contains the same convex
            combination of the two points, so it is non-empty and the return constraint is active for a minimum-risk x.

    Also returns the demo's constraint as matrices: c(x) = A x - b with A = [mu'; e'], b = 0 (demo/portfolio.jl:43-56) and
    D = [rho, inf) x {1} as vector bounds lo, hi (:58-66)."""
    r = max(1, n // 10) if rank is None else int(rank)
    F = 0.2 * (2.0 * uniform(1, n * r) - 1.0).reshape(n, r)
    d = 0.01 + 0.04 * uniform(2, n)
    Q = F @ F.T + np.diag(d)
    Q = 0.5 * (Q + Q.T)
    mu = 0.1 * uniform(3, n)
    ub = (2.0 + 6.0 * uniform(4, n)) / n
    xfeas = ub / ub.sum()
    order = np.argsort(-mu, kind="stable")
    room = 1.0 - np.concatenate(([0.0], np.cumsum(ub[order])[:-1]))
    xbest = np.zeros(n)
    xbest[order] = np.clip(room, 0.0, ub[order])
    rho = 0.75 * float(mu @ xfeas) + 0.25 * float(mu @ xbest)
    A = np.stack([mu, np.ones(n)])
    return {"Q": Q.astype(dtype), "mu": mu.astype(dtype), "ub": ub.astype(dtype), "rho": float(np.dtype(dtype).type(rho)),
            "A": np.ascontiguousarray(A.astype(dtype)), "b": np.zeros(2, dtype),
            "lo": np.array([rho, 1.0], dtype), "hi": np.array([np.inf, 1.0], dtype),
            "xfeas": (0.75 * xfeas + 0.25 * xbest).astype(dtype)}
