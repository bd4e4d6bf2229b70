"""The f/g/c/D oracle types of Bazinga.alps that this build lowers to the device.

The reference's oracles are duck-typed Julia structs (README.md:17-20,
src/Bazinga.jl:7-16).  A device cannot run arbitrary closures, so the host side
pattern-matches the structured types below and lowers them to a C descriptor
(`bz_problem_desc`, include/bazinga_hip.h).

Anything else is a GENERIC oracle (demo/rosenbrock.jl:39-80 — BASELINE config 1): an object with
the reference's protocol

    f.gradient(dfx, x) -> f(x)        gradient!(dfx, f, x)       src/Bazinga.jl:16
    g.prox(z, x, gamma) -> g(z)       prox!(z, g, x, gamma)      src/Bazinga.jl:15
    c.eval(cx, x), c.jtprod(jtv, x, v)                           src/Bazinga.jl:11-12
    D.proj(s, v)                      proj!(s, D, v)             src/Bazinga.jl:14

is handed to the library as host callbacks (BZ_*_CALLBACK): the host evaluates the oracles, the
device keeps the L-BFGS / line-search vector work.  When one of the four is generic all four travel
as callbacks (the structured types below carry the same protocol for that case).  An object with
neither raises ``UnsupportedOracle``; nothing ever falls back to a CPU solver.
"""
from __future__ import annotations

import numpy as np

import ctypes as C

from . import _lib as L


class UnsupportedOracle(TypeError):
    pass


# ----------------------------------------------------------------- abstract tags
class ProximableFunction:   # src/Bazinga.jl:7
    pass


class SmoothFunction:       # src/Bazinga.jl:8
    pass


class ClosedSetBase:        # src/Bazinga.jl:9  (abstract type ClosedSet)
    pass


# ------------------------------------------------------------------------- f
class Zero(ProximableFunction):
    """src/proxoperators/zero.jl:11-25; usable as f or g."""

    def gradient(self, dfx, x):
        dfx[...] = 0
        return x.dtype.type(0)

    def prox(self, z, x, gamma):
        z[...] = x
        return x.dtype.type(0)


class DiagQuadratic(ProximableFunction):
    """f(x) = sum_i x_i (0.5 q_i x_i - b_i) — diagonal special case of
    ProximalOperators.Quadratic (test/problems/test_nonconvex_qp.jl:14)."""

    def __init__(self, q, b):
        self.q = np.ascontiguousarray(q)
        self.b = np.ascontiguousarray(b)
        if self.q.shape != self.b.shape or self.q.ndim != 1:
            raise ValueError("q and b must be vectors of equal length")

    def gradient(self, dfx, x):
        qx = self.q * x
        dfx[...] = qx - self.b
        return np.sum(x * (x.dtype.type(0.5) * qx - self.b))


class LeastSquares(ProximableFunction):
    """ProximalOperators.LeastSquares(A, b): f(x) = 0.5||A x - b||^2 (test/problems/test_verbose.jl:22)."""

    def __init__(self, A, b):
        self.A = np.ascontiguousarray(A)
        self.b = np.ascontiguousarray(b)
        if self.A.ndim != 2 or self.b.shape != (self.A.shape[0],):
            raise ValueError("A must be m-by-n and b of length m")

    def gradient(self, dfx, x):
        r = self.A @ x - self.b
        dfx[...] = self.A.T @ r
        return x.dtype.type(0.5) * np.dot(r, r)


class Quadratic(ProximableFunction):
    """ProximalOperators.Quadratic(Q, q): f(x) = 0.5 x'Qx + q'x, Q dense symmetric
    (test/problems/test_nonconvex_qp.jl:14,65)."""

    def __init__(self, Q, q):
        self.Q = np.ascontiguousarray(Q)
        self.q = np.ascontiguousarray(q)
        if self.Q.ndim != 2 or self.Q.shape[0] != self.Q.shape[1] or self.q.shape != (self.Q.shape[0],):
            raise ValueError("Q must be n-by-n and q of length n")

    def gradient(self, dfx, x):
        Qx = self.Q @ x
        dfx[...] = Qx + self.q
        return x.dtype.type(0.5) * np.dot(x, Qx) + np.dot(self.q, x)


_REALS = (np.float64, np.float32)
_I32_MAX = 2 ** 31 - 1


def _real_array(a, name, dtype):
    """labels, b or weights as a contiguous real array: float64 / float32 as given, integers taking `dtype` (that of data)"""
    a = np.asarray(a)
    if not (np.issubdtype(a.dtype, np.integer) or a.dtype in _REALS):
        raise ValueError(f"{name} must be float64, float32 or integers")
    return np.asarray(a, dtype=dtype if np.issubdtype(a.dtype, np.integer) else a.dtype, order="C")


class _CSR:
    """What the six classes below that carry a CSR matrix share: its validation in two steps (`_csr_types` before a class's
    own checks of b / labels, `_csr_shape` after them, so that the first error of a faulty input is the same in every class),
    the matrix methods, and the two products."""

    def _csr_types(self, indptr, indices, data, other, name, both=False):
        """step one: one-dimensional arrays (`other`, called `name` in the messages, is q, b or the labels), integer
        indptr / indices, a float64 / float32 data (both=True: and `other`)"""
        ip, ix = np.asarray(indptr), np.asarray(indices)
        self.data = np.ascontiguousarray(data)
        if ip.ndim != 1 or ix.ndim != 1 or self.data.ndim != 1 or other.ndim != 1:
            raise ValueError(f"indptr, indices, data and {name} must be one-dimensional")
        if not (np.issubdtype(ip.dtype, np.integer) and np.issubdtype(ix.dtype, np.integer)):
            raise ValueError("indptr and indices must be integer arrays")
        if self.data.dtype not in _REALS or (both and other.dtype not in _REALS):
            raise ValueError(f"data{' and ' + name if both else ''} must be float64 or float32")
        self.indptr, self.indices = ip, ix                   # (as given until _csr_shape has checked them)

    def _csr_shape(self, rows, cols, rows_name):
        """step two: indptr / indices against `rows` (called `rows_name` in the message) and `cols`, then their int64 /
        int32 forms and the row of every entry"""
        ip, ix = self.indptr, self.indices
        if ip.shape[0] != rows + 1:
            raise ValueError(f"indptr must have length {rows_name} + 1 = {rows + 1}")
        if ix.shape[0] != self.data.shape[0]:
            raise ValueError("indices and data must have the same length")
        if ip[0] != 0 or ip[-1] != ix.shape[0] or np.any(np.diff(ip) < 0):
            raise ValueError("indptr must start at 0, be non-decreasing and end at nnz")
        if ix.shape[0] and (ix.min() < 0 or ix.max() >= cols):
            raise ValueError(f"column indices must lie in [0, {cols})")
        self.indptr = np.ascontiguousarray(ip, dtype=np.int64)
        self.indices = np.ascontiguousarray(ix, dtype=np.int32)
        self._shape = (rows, cols)
        self._rows = np.repeat(np.arange(rows, dtype=np.int64), np.diff(self.indptr))      # the row of every entry

    @property
    def nnz(self):
        return int(self.indices.shape[0])

    @staticmethod
    def _csr_of_dense(A, what, square=False):
        """((indptr, indices, data), columns) of the non-zeros of a dense matrix; `what` is the class's "A must be ..." """
        A = np.asarray(A)
        if A.ndim != 2 or (square and A.shape[0] != A.shape[1]):
            raise ValueError(what)
        mask = A != 0
        indptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1)))).astype(np.int64)
        indices = np.nonzero(mask)[1].astype(np.int32)
        return (indptr, indices, np.ascontiguousarray(A[mask])), A.shape[1]

    @staticmethod
    def _csr_of_scipy(M):
        """the same of any scipy.sparse matrix (scipy is imported here and nowhere else: it is not a dependency)"""
        import scipy.sparse as sp
        M = sp.csr_matrix(M)
        return (M.indptr, M.indices, M.data), M.shape[1]

    def toarray(self):
        A = np.zeros(self._shape, self.data.dtype)
        np.add.at(A, (self._rows, self.indices), self.data)
        return A

    def _matvec(self, x):
        """A x: the float64 sums, not rounded (every caller rounds where its formula does)"""
        return np.bincount(self._rows, weights=self.data * x[self.indices], minlength=self._shape[0])

    def _rmatvec(self, v):
        """A'v, as _matvec"""
        return np.bincount(self.indices, weights=self.data * v[self._rows], minlength=self._shape[1])


class _RowWeighted:
    """`weights` and `scale` of SparseGLM and SparseMultinomial: a weight per row (w[m] >= 0, or None) and one number > 0"""

    def _set_row_weights(self, weights, scale):
        if not (np.ndim(scale) == 0 and np.isfinite(scale) and scale > 0):
            raise ValueError("scale must be a finite number > 0")
        self.scale = float(scale)
        self.weights = None
        if weights is not None:
            w = _real_array(weights, "weights", self.data.dtype)
            if w.shape != (self.m,) or not np.all(np.isfinite(w) & (w >= 0)):
                raise ValueError(f"weights must be {self.m} finite numbers >= 0")
            self.weights = w

    def row_weights(self, dtype):
        """w^ in dtype: scale * w with the product in float64, rounded once (without weights the one number scale)"""
        dt = np.dtype(dtype).type
        with np.errstate(over="ignore"):                 # (a product beyond the dtype's range rounds to inf: lower() refuses it)
            if self.weights is None:
                return dt(self.scale)
            return (self.scale * self.weights.astype(np.float64)).astype(dt)


class SparseQuadratic(_CSR, ProximableFunction):
    """ProximalOperators.Quadratic(Q, q) with a sparse Q: f(x) = 0.5 x'Qx + q'x, Q symmetric n-by-n in CSR (indptr[n + 1],
    indices[nnz] 0-based, data[nnz]), never densified.  The conventions of SparseAffine: the column indices of a row
    need not be sorted, an index that occurs twice in a row contributes twice, an empty row gives (Qx)_i = 0.  Symmetry
    is the caller's contract on the device; check_symmetric=True compares the summed (row, col) -> value maps of Q and
    Q' exactly here.  __call__ / gradient below are numpy with ref.Quadratic's formulas (the host outer loop, and the
    generic-oracle protocol); on the device the kind is BZ_F_SPARSE_QUADRATIC."""

    def __init__(self, indptr, indices, data, q, *, check_symmetric=True):
        self.q = np.ascontiguousarray(q)
        self._csr_types(indptr, indices, data, self.q, "q", both=True)
        self.n = self.q.shape[0]
        if self.n <= 0 or self.n > _I32_MAX:
            raise ValueError("n must be in 1 .. 2^31 - 1")
        self._csr_shape(self.n, self.n, "n")
        if check_symmetric and not self._is_symmetric():
            raise ValueError("Q must be symmetric (the summed entries of Q and Q' differ)")

    def _is_symmetric(self):
        """the (row, col) -> summed value maps of Q and Q', compared exactly (the sums in float64, entry order)"""
        def summed(r, c):
            key = r * self.n + c
            u, inv = np.unique(key, return_inverse=True)
            return u, np.bincount(inv, weights=self.data.astype(np.float64), minlength=u.shape[0])
        cols = self.indices.astype(np.int64)
        (ka, va), (kb, vb) = summed(self._rows, cols), summed(cols, self._rows)
        if np.array_equal(ka, kb):
            return bool(np.array_equal(va, vb))
        # (an entry stored on one side only counts as a zero on the other)
        keys = np.union1d(ka, kb)
        fa, fb = np.zeros(keys.shape[0]), np.zeros(keys.shape[0])
        fa[np.searchsorted(keys, ka)] = va
        fb[np.searchsorted(keys, kb)] = vb
        return bool(np.array_equal(fa, fb))

    @classmethod
    def from_dense(cls, Q, q, **kw):
        csr, _ = cls._csr_of_dense(Q, "Q must be n-by-n", square=True)
        return cls(*csr, q, **kw)

    @classmethod
    def from_scipy(cls, M, q, **kw):
        return cls(*cls._csr_of_scipy(M)[0], q, **kw)

    def _Qx(self, x):
        return self._matvec(x).astype(x.dtype, copy=False)

    def __call__(self, x):
        return x.dtype.type(0.5) * np.dot(x, self._Qx(x)) + np.dot(x, self.q)

    def gradient(self, dfx, x):
        dfx[...] = self._Qx(x)
        fx = x.dtype.type(0.5) * np.dot(x, dfx)
        dfx += self.q
        return fx + np.dot(x, self.q)


class SparseLeastSquares(_CSR, ProximableFunction):
    """ProximalOperators.LeastSquares(A, b) with a sparse A: f(x) = 0.5||A x - b||^2, A m-by-n in CSR (indptr[m + 1],
    indices[nnz] 0-based, data[nnz]), never densified and never squared into A'A.  The conventions of SparseAffine: the
    column indices of a row need not be sorted, an index that occurs twice in a row contributes twice, an empty row gives
    r_i = -b_i and an empty column a zero gradient entry; nnz = 0 is accepted.  __call__ / gradient below are numpy with
    ref.LeastSquares' formulas (the generic-oracle protocol); on the device the kind is BZ_F_SPARSE_LEAST_SQUARES."""

    def __init__(self, indptr, indices, data, b, n):
        self.b = np.ascontiguousarray(b)
        self.n = int(n)
        self._csr_types(indptr, indices, data, self.b, "b", both=True)
        self.m = self.b.shape[0]
        if self.n <= 0 or self.n > _I32_MAX or self.m <= 0 or self.m > _I32_MAX:
            raise ValueError("n and the length of b must be in 1 .. 2^31 - 1")
        self._csr_shape(self.m, self.n, "m")

    @classmethod
    def from_dense(cls, A, b):
        csr, n = cls._csr_of_dense(A, "A must be m-by-n")
        return cls(*csr, b, n)

    @classmethod
    def from_scipy(cls, M, b):
        csr, n = cls._csr_of_scipy(M)
        return cls(*csr, b, n)

    def _residual(self, x):
        return (self._matvec(x) - self.b).astype(x.dtype, copy=False)

    def __call__(self, x):
        r = self._residual(x)
        return x.dtype.type(0.5) * np.dot(r, r)

    def gradient(self, dfx, x):
        r = self._residual(x)
        dfx[...] = self._rmatvec(r)
        return x.dtype.type(0.5) * np.dot(r, r)


class SparseLogistic(_CSR, ProximableFunction):
    """The logistic loss of a sparse design matrix: f(x) = sum_i log(1 + exp(-b_i a_i'x)), A m-by-n in CSR (indptr[m + 1],
    indices[nnz] 0-based, data[nnz]), labels b in {-1, +1}^m, never densified.  The plain sum: no 1/2 and no 1/m.  The matrix
    conventions of SparseLeastSquares (unsorted and repeated column indices, empty rows and columns, nnz = 0).  With
    u = b_i a_i'x the row's loss is softplus(-u) = max(-u, 0) + log1p(exp(-|u|)) and the gradient is A'r with
    r_i = -b_i sigma(-u), sigma(-u) = e / (1 + e) for u >= 0 and 1 / (1 + e) otherwise, e = exp(-|u|): nothing overflows,
    nothing cancels, and a NaN in u reaches both.  __call__ / gradient below are numpy with these formulas in the dtype of x
    (the generic-oracle protocol); on the device the kind is BZ_F_SPARSE_LOGISTIC."""

    def __init__(self, indptr, indices, data, labels, n):
        lab = np.asarray(labels)
        self.n = int(n)
        self._csr_types(indptr, indices, data, lab, "labels")
        self.b = _real_array(lab, "labels", self.data.dtype)
        if not np.all(np.abs(self.b) == 1):
            raise ValueError("labels must be -1 or +1")
        self.m = self.b.shape[0]
        if self.n <= 0 or self.n > _I32_MAX or self.m <= 0 or self.m > _I32_MAX:
            raise ValueError("n and the number of labels must be in 1 .. 2^31 - 1")
        self._csr_shape(self.m, self.n, "m")

    @classmethod
    def from_dense(cls, A, labels):
        csr, n = cls._csr_of_dense(A, "A must be m-by-n")
        return cls(*csr, labels, n)

    @classmethod
    def from_scipy(cls, M, labels):
        csr, n = cls._csr_of_scipy(M)
        return cls(*csr, labels, n)

    def _loss_r(self, x):
        """the rows' losses softplus(-u) and r = -b sigma(-u), u = b * (A x), in the dtype of x"""
        dt = x.dtype.type
        t = self._matvec(x).astype(x.dtype, copy=False)
        b = self.b.astype(x.dtype, copy=False)
        u = b * t
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-np.abs(u))
            loss = np.where(u < 0, -u, dt(0)) + np.log1p(e)
            s = np.where(u >= 0, e / (dt(1) + e), dt(1) / (dt(1) + e))
        return loss, -b * s

    def __call__(self, x):
        return x.dtype.type(np.sum(self._loss_r(x)[0]))

    def gradient(self, dfx, x):
        loss, r = self._loss_r(x)
        dfx[...] = self._rmatvec(r)
        return x.dtype.type(np.sum(loss))


class SparseGLM(_CSR, _RowWeighted, ProximableFunction):
    """A row loss of a sparse design matrix with a weight per row: f(x) = sum_i w^_i l(b_i, t_i), t = A x, w^_i = scale * w_i,
    A m-by-n in CSR (indptr[m + 1], indices[nnz] 0-based, data[nnz]), never densified; the gradient is A'r with
    r_i = w^_i dl/dt(b_i, t_i).  The matrix conventions of SparseLeastSquares (unsorted and repeated column indices, empty rows
    and columns, nnz = 0; an empty row has t = 0).  `loss`, with v = t - b and u = b t:
      "least_squares"  l = v^2 / 2, l' = v (the 1/2 is taken on the sum)
      "logistic"       b = +-1: SparseLogistic's l = softplus(-u), l' = -b sigma(-u)
      "huber"          delta > 0: |v| <= delta: l = v^2 / 2, l' = v ; otherwise l = delta (|v| - delta / 2), l' = +-delta
      "squared_hinge"  b = +-1, h = 1 - u: h <= 0: l = l' = 0 ; otherwise l = h^2 / 2, l' = -b h
      "poisson"        counts b >= 0, log link, without the constant log b!: e = exp(t), l = e - b t (b = 0: l = e ; where e has
                       overflowed l = +inf, never inf - inf), l' = e - b
    Ordered compares and arithmetic alone: a NaN in t reaches the loss and r.  `weights` (w[m] >= 0, or None) and `scale` (> 0;
    1 / m gives the mean) are folded into one number per row, the product in float64 rounded once to the dtype; the row's term
    is w^ * l and r = w^ * l', one multiplication each.  __call__ / gradient below are numpy with these formulas in the dtype
    of x (the generic-oracle protocol); on the device the kind is BZ_F_SPARSE_GLM."""

    LOSSES = ("least_squares", "logistic", "huber", "squared_hinge", "poisson")

    def __init__(self, indptr, indices, data, b, n, loss, delta=None, weights=None, scale=1.0):
        bb = np.asarray(b)
        self.n = int(n)
        if loss not in self.LOSSES:
            raise ValueError(f"unknown loss {loss!r}: one of {self.LOSSES}")
        self.loss = loss
        self._csr_types(indptr, indices, data, bb, "b")
        self.b = _real_array(bb, "b", self.data.dtype)
        if loss in ("logistic", "squared_hinge") and not np.all(np.abs(self.b) == 1):
            raise ValueError(f"labels must be -1 or +1 for the {loss} loss")
        if loss == "poisson" and not np.all(np.isfinite(self.b) & (self.b >= 0)):
            raise ValueError("counts must be finite and >= 0 for the poisson loss")
        if loss == "huber":
            if delta is None or not (np.isfinite(delta) and delta > 0):
                raise ValueError("the huber loss needs delta finite and > 0")
        elif delta is not None:
            raise ValueError(f"delta is the huber loss's parameter, not the {loss} loss's")
        self.delta = None if delta is None else float(delta)
        self.m = self.b.shape[0]
        if self.n <= 0 or self.n > _I32_MAX or self.m <= 0 or self.m > _I32_MAX:
            raise ValueError("n and the length of b must be in 1 .. 2^31 - 1")
        self._set_row_weights(weights, scale)
        self._csr_shape(self.m, self.n, "m")

    @classmethod
    def from_dense(cls, A, b, loss, **kw):
        csr, n = cls._csr_of_dense(A, "A must be m-by-n")
        return cls(*csr, b, n, loss, **kw)

    @classmethod
    def from_scipy(cls, M, b, loss, **kw):
        csr, n = cls._csr_of_scipy(M)
        return cls(*csr, b, n, loss, **kw)

    @staticmethod
    def loss_and_derivative(loss, delta, b, t):
        """the rows' l(b, t) and dl/dt(b, t) in the dtype of t (least_squares: v^2, the 1/2 being taken on the sum)"""
        dt = t.dtype.type
        with np.errstate(over="ignore", invalid="ignore"):
            if loss == "least_squares":
                v = t - b
                return v * v, v
            if loss == "logistic":
                u = b * t
                e = np.exp(-np.abs(u))
                s = np.where(u >= 0, e / (dt(1) + e), dt(1) / (dt(1) + e))
                return np.where(u < 0, -u, dt(0)) + np.log1p(e), -b * s
            if loss == "huber":
                v, d = t - b, dt(delta)
                a = np.where(v < 0, -v, v)
                inside = a <= d
                return (np.where(inside, dt(0.5) * v * v, d * (a - dt(0.5) * d)),
                        np.where(inside, v, np.where(v > 0, d, np.where(v < 0, -d, v))))
            if loss == "squared_hinge":
                h = dt(1) - b * t
                off = h <= 0
                return np.where(off, dt(0), dt(0.5) * h * h), np.where(off, dt(0), -b * h)
            e = np.exp(t)
            bt = np.where(b == 0, dt(0), b * t)
            return np.where(e < np.inf, e - bt, e), e - b

    def _loss_r(self, x):
        """the rows' terms w^ l (least_squares: w^ v^2) and r = w^ l' in the dtype of x"""
        t = self._matvec(x).astype(x.dtype, copy=False)
        l, dl = self.loss_and_derivative(self.loss, self.delta, self.b.astype(x.dtype, copy=False), t)
        w = self.row_weights(x.dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            return w * l, w * dl

    def _value(self, terms, dt):
        fx = dt(np.sum(terms))
        return dt(0.5) * fx if self.loss == "least_squares" else fx

    def __call__(self, x):
        return self._value(self._loss_r(x)[0], x.dtype.type)

    def gradient(self, dfx, x):
        terms, r = self._loss_r(x)
        dfx[...] = self._rmatvec(r)
        return self._value(terms, x.dtype.type)


class SparseMultinomial(_CSR, _RowWeighted, ProximableFunction):
    """Multinomial (softmax) regression on a sparse design matrix: f(X) = sum_i w^_i (logsumexp_k(t_ik) - t_{i,b_i}), T = A X,
    w^_i = scale * w_i; A m-by-n_features in CSR (indptr[m + 1], indices[nnz] 0-based, data[nnz]), never densified; labels b in
    {0 .. K - 1}^m, K = n_classes in 2 .. 64.  X is n_features x K ROW-MAJOR (class fastest): the variable is the flat vector x of
    length n = n_features * K with x[j * K + k] = X[j, k] (`coef(x)` is that view).  The symmetric, over-parameterised softmax, as
    glmnet has it: no reference class.  The gradient is A'R, laid out as X is, with r_ik = w^_i (p_ik - [k = b_i]).  Per row, with
    ordered compares and arithmetic alone: mx = max_k t_ik, e_k = exp(t_ik - mx), S = sum_k e_k, p_k = e_k / S, and the row's loss
    is w^_i ((mx - t_{i,b_i}) + log S).  A NaN in any t_ik reaches the row's loss and all K of its r; t_ik = +inf gives NaN
    (inf - inf); an empty row has t = 0: loss w^_i log K, p = 1 / K.  The matrix conventions of SparseLeastSquares; `weights` and
    `scale` as SparseGLM has them (the product in float64, rounded once to the dtype).  __call__ / gradient below are numpy with
    these formulas in the dtype of x (the generic-oracle protocol); on the device the kind is BZ_F_SPARSE_MULTINOMIAL.
    The first step size: PANOCplus estimates it from grad L(x0 + 1) - grad L(x0), and adding one number to all K classes of a
    feature leaves f unchanged; where the penalty is flat there too (D = FreeSet, a box holding x0 and x0 + 1) the estimate is 0
    and gamma = alpha / 0, as in the reference's algorithm.  Give the step size: PANOCplus(gamma=1.0, adaptive=True), or Lf."""

    def __init__(self, indptr, indices, data, labels, n_features, n_classes, weights=None, scale=1.0):
        lab = np.asarray(labels)
        self.n_features, self.n_classes = int(n_features), int(n_classes)
        if not 2 <= self.n_classes <= 64:
            raise ValueError("n_classes must be in 2 .. 64")
        self._csr_types(indptr, indices, data, lab, "labels")
        self.b = lab = _real_array(lab, "labels", self.data.dtype)
        with np.errstate(invalid="ignore"):
            if not np.all(np.isfinite(lab) & (lab == np.floor(lab)) & (lab >= 0) & (lab < self.n_classes)):
                raise ValueError(f"labels must be integers in [0, {self.n_classes})")
        self.m = self.b.shape[0]
        self.n = self.n_features * self.n_classes
        if self.n_features <= 0 or self.n > _I32_MAX or self.m <= 0 or self.m > _I32_MAX:
            raise ValueError("n_features * n_classes and the number of labels must be in 1 .. 2^31 - 1")
        self._set_row_weights(weights, scale)
        self._csr_shape(self.m, self.n_features, "m")

    @classmethod
    def from_dense(cls, A, labels, n_classes, **kw):
        csr, n_features = cls._csr_of_dense(A, "A must be m-by-n_features")
        return cls(*csr, labels, n_features, n_classes, **kw)

    @classmethod
    def from_scipy(cls, M, labels, n_classes, **kw):
        csr, n_features = cls._csr_of_scipy(M)
        return cls(*csr, labels, n_features, n_classes, **kw)

    def coef(self, x):
        """the (n_features, n_classes) view of the flat variable"""
        return np.asarray(x).reshape(self.n_features, self.n_classes)

    @staticmethod
    def softmax_terms(t, labels, w):
        """the rows' losses w ((mx - t_b) + log S) and R = w (p - onehot(b)) from T (m x K) in its dtype"""
        dt = t.dtype.type
        rows = np.arange(t.shape[0])
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            mx = np.max(t, axis=1)
            e = np.exp(t - mx[:, None])
            S = np.sum(e, axis=1, dtype=t.dtype)
            r = e / S[:, None]
            r[rows, labels] -= dt(1)
            w = np.asarray(w, t.dtype)
            loss = w * ((mx - t[rows, labels]) + np.log(S))
            return loss, (w[:, None] if w.ndim else w) * r

    def _loss_r(self, x):
        K = self.n_classes
        X = self.coef(x)
        t = np.zeros((self.m, K), x.dtype)
        np.add.at(t, self._rows, self.data.astype(x.dtype, copy=False)[:, None] * X[self.indices])
        return self.softmax_terms(t, self.b.astype(np.int64), self.row_weights(x.dtype))

    def __call__(self, x):
        return x.dtype.type(np.sum(self._loss_r(x)[0]))

    def gradient(self, dfx, x):
        loss, r = self._loss_r(x)
        G = np.zeros((self.n_features, self.n_classes), x.dtype)
        np.add.at(G, self.indices, self.data.astype(x.dtype, copy=False)[:, None] * r[self._rows])
        dfx[...] = G.reshape(-1)
        return x.dtype.type(np.sum(loss))


class SparseMultiGLM(_CSR, _RowWeighted, ProximableFunction):
    """K independent row losses of one sparse design matrix: f(X) = sum_i w^_i sum_k l(B_ik, t_ik), T = A X, w^_i = scale * w_i;
    A m-by-n_features in CSR (indptr[m + 1], indices[nnz] 0-based, data[nnz]), never densified; B is (m, K), K in 2 .. 64 (a
    vector b is SparseGLM's).  Multi-response regression with "least_squares" (0.5 ||A X - B||_F^2; with NormL21(lam, group=K) the
    multi-task Lasso), multi-label classification with "logistic" or "squared_hinge" and B in {-1, +1}.  X is n_features x K
    ROW-MAJOR (response fastest), as SparseMultinomial has it: the variable is the flat vector x of length n = n_features * K with
    x[j * K + k] = X[j, k] (`coef(x)` is that view).  `loss`, `delta`, `weights` and `scale` are SparseGLM's, with its formulas and
    its checks applied to every entry of B; a weight belongs to a ROW and is shared by its K responses.  The gradient is A'R, laid
    out as X is, with r_ik = w^_i dl/dt(B_ik, t_ik); the K responses of a row exchange nothing.  The matrix conventions of
    SparseLeastSquares.  __call__ / gradient below are numpy with SparseGLM.loss_and_derivative on T in the dtype of x (the
    generic-oracle protocol); on the device the kind is BZ_F_SPARSE_MULTI_GLM.  Every loss sees PANOCplus' step-size probe
    x0 + 1, so the default PANOCplus() needs no gamma."""

    LOSSES = SparseGLM.LOSSES

    def __init__(self, indptr, indices, data, B, n_features, loss, delta=None, weights=None, scale=1.0):
        bb = np.asarray(B)
        self.n_features = int(n_features)
        if loss not in self.LOSSES:
            raise ValueError(f"unknown loss {loss!r}: one of {self.LOSSES}")
        self.loss = loss
        if bb.ndim == 1:
            raise ValueError("B must be (m, K) with K >= 2 responses per row: a vector b is SparseGLM's")
        if bb.ndim != 2:
            raise ValueError("B must be two-dimensional, (m, K)")
        self.n_classes = int(bb.shape[1])
        if not 2 <= self.n_classes <= 64:
            raise ValueError("B must have K in 2 .. 64 columns (K = 1 is SparseGLM)")
        self._csr_types(indptr, indices, data, bb.reshape(-1), "B")
        self.B = _real_array(bb, "B", self.data.dtype)
        if loss in ("logistic", "squared_hinge") and not np.all(np.abs(self.B) == 1):
            raise ValueError(f"labels must be -1 or +1 for the {loss} loss")
        if loss == "poisson" and not np.all(np.isfinite(self.B) & (self.B >= 0)):
            raise ValueError("counts must be finite and >= 0 for the poisson loss")
        if loss == "huber":
            if delta is None or not (np.isfinite(delta) and delta > 0):
                raise ValueError("the huber loss needs delta finite and > 0")
        elif delta is not None:
            raise ValueError(f"delta is the huber loss's parameter, not the {loss} loss's")
        self.delta = None if delta is None else float(delta)
        self.m = self.B.shape[0]
        self.n = self.n_features * self.n_classes
        if self.n_features <= 0 or self.n > _I32_MAX or self.m <= 0 or self.m > _I32_MAX:
            raise ValueError("n_features * K and the number of rows of B must be in 1 .. 2^31 - 1")
        self._set_row_weights(weights, scale)
        self._csr_shape(self.m, self.n_features, "m")

    @property
    def b(self):
        """B as f_b holds it: the flat row-major vector, b[i * K + k] = B[i, k]"""
        return self.B.reshape(-1)

    @classmethod
    def from_dense(cls, A, B, loss, **kw):
        csr, n_features = cls._csr_of_dense(A, "A must be m-by-n_features")
        return cls(*csr, B, n_features, loss, **kw)

    @classmethod
    def from_scipy(cls, M, B, loss, **kw):
        csr, n_features = cls._csr_of_scipy(M)
        return cls(*csr, B, n_features, loss, **kw)

    def coef(self, x):
        """the (n_features, K) view of the flat variable"""
        return np.asarray(x).reshape(self.n_features, self.n_classes)

    def _loss_r(self, x):
        """the terms w^ l (least_squares: w^ v^2) and R = w^ l', both (m, K), in the dtype of x"""
        X = self.coef(x)
        t = np.stack([self._matvec(X[:, k]) for k in range(self.n_classes)], axis=1).astype(x.dtype, copy=False)
        l, dl = SparseGLM.loss_and_derivative(self.loss, self.delta, self.B.astype(x.dtype, copy=False), t)
        w = self.row_weights(x.dtype)
        w = w[:, None] if np.ndim(w) else w
        with np.errstate(over="ignore", invalid="ignore"):
            return w * l, w * dl

    def _value(self, terms, dt):
        fx = dt(np.sum(terms))
        return dt(0.5) * fx if self.loss == "least_squares" else fx

    def __call__(self, x):
        return self._value(self._loss_r(x)[0], x.dtype.type)

    def gradient(self, dfx, x):
        terms, r = self._loss_r(x)
        dfx[...] = np.stack([self._rmatvec(r[:, k]) for k in range(self.n_classes)], axis=1).reshape(-1)
        return self._value(terms, x.dtype.type)


class Stencil5ptQuadratic(ProximableFunction):
    """f(x) = 0.5 x'A_h x - b'x on an nx-by-ny grid (row-major), A_h the 5-point Laplacian
    (4,-1,-1,-1,-1) with homogeneous Dirichlet halo — the structured `Quadratic` of BASELINE
    config 3; 1-D analogue in the reference: demo/obstacle.jl:97-112."""

    def __init__(self, nx, ny, b):
        self.nx, self.ny = int(nx), int(ny)
        self.b = np.ascontiguousarray(b)
        if self.b.shape != (self.nx * self.ny,):
            raise ValueError("b must have length nx*ny")


# ------------------------------------------------------------------------- g
class IndFree(ProximableFunction):
    """ProximalOperators.IndFree (test_nonconvex_qp.jl:39)."""

    def prox(self, z, x, gamma=1.0):
        z[...] = x
        return x.dtype.type(0)


class NormL1(ProximableFunction):
    """ProximalOperators.NormL1(lambda) (test_verbose.jl:23, demo/basispursuit.jl:63).  lambda is a number, or a 1-D
    array of per-element weights, g(x) = sum lambda_i |x_i| (finite, >= 0; a zero leaves its coefficient unpenalised)."""

    def __init__(self, lam=1.0):
        if np.ndim(lam) == 0:
            if lam < 0:
                raise ValueError("parameter λ must be nonnegative")
            self.lam = float(lam)
            return
        lam = np.array(lam, dtype=np.float64)
        if lam.ndim != 1:
            raise ValueError("parameter λ must be a number or a 1-D array")
        if not np.all(np.isfinite(lam) & (lam >= 0)):
            raise ValueError("parameter λ must have finite, nonnegative entries")
        self.lam = lam

    def __call__(self, x):
        return np.sum(np.abs(self.lam * x)) if np.ndim(self.lam) else self.lam * np.sum(np.abs(x))

    def prox(self, z, x, gamma):
        T = x.dtype.type
        if np.ndim(self.lam) == 0:
            gl = T(gamma * self.lam)
            z[...] = x + np.where(x <= -gl, gl, np.where(x >= gl, -gl, -x))
            return T(self.lam) * np.sum(np.abs(z))
        lam = np.asarray(self.lam, dtype=x.dtype)
        gl = T(gamma) * lam
        z[...] = x + np.where(x <= -gl, gl, np.where(x >= gl, -gl, -x))
        return np.sum(lam * np.abs(z))


class ElasticNet(ProximableFunction):
    """ProximalOperators.ElasticNet(mu, lambda) with penalty factors: g(x) = sum_i w_i (l1 |x_i| + l2/2 x_i^2), l1 and l2
    finite and >= 0, `weights` a 1-D array of finite entries >= 0 or None (every w_i = 1; a zero leaves its element wholly
    unpenalised: an intercept).  glmnet's penalty lambda sum pf_j (alpha |b_j| + (1 - alpha)/2 b_j^2) is
    ElasticNet.glmnet(lam, alpha, penalty_factor).  `prox` restates the device's arm (include/bazinga_hip.h,
    BZ_G_ELASTIC_NET) operation for operation in the type of x, so it gives the device's bits."""

    def __init__(self, l1=1.0, l2=1.0, weights=None):
        for name, v in (("l1", l1), ("l2", l2)):
            if np.ndim(v) != 0 or not (np.isfinite(v) and v >= 0):
                raise ValueError(f"parameter {name} must be a finite, nonnegative number")
        self.l1, self.l2 = float(l1), float(l2)
        if weights is not None:
            weights = np.array(weights, dtype=np.float64)
            if weights.ndim != 1:
                raise ValueError("weights must be None or a 1-D array")
            if not np.all(np.isfinite(weights) & (weights >= 0)):
                raise ValueError("weights must have finite, nonnegative entries")
        self.weights = weights

    @classmethod
    def glmnet(cls, lam, alpha, penalty_factor=None):
        """glmnet's parametrisation: l1 = lam * alpha, l2 = lam * (1 - alpha), weights = penalty.factor"""
        if np.ndim(alpha) != 0 or not (0 <= alpha <= 1):
            raise ValueError("alpha must be a number in [0, 1]")
        return cls(lam * alpha, lam * (1 - alpha), penalty_factor)

    def _check(self, dtype):
        """the C side's rule for the problem's type: neither number above its largest"""
        if max(self.l1, self.l2) > float(np.finfo(dtype).max):
            raise ValueError(f"l1 and l2 must be finite in {np.dtype(dtype)}")

    def __call__(self, x):
        term = self.l1 * np.abs(x) + (0.5 * self.l2) * (x * x)
        return np.sum(term if self.weights is None else self.weights * term)

    def prox(self, z, x, gamma):
        T = x.dtype.type
        l1, l2 = T(self.l1), T(self.l2)
        w = None if self.weights is None else np.asarray(self.weights, dtype=x.dtype)
        with np.errstate(all="ignore"):
            t = T(gamma) if w is None else T(gamma) * w
            a = t * l1
            d = T(1) + t * l2
            # y - min(max(y, -a), a): NormL1's expression (its `where` form has the same bits for every y and a, the
            # signed zeros, infinities and NaN included)
            s = x + np.where(x <= -a, a, np.where(x >= a, -a, -x))
            z[...] = s / d
            term = l1 * np.abs(z) + (T(0.5) * l2) * (z * z)
            if w is not None:
                term = w * term
            return np.sum(term)


class NormL21(ProximableFunction):
    """The group Lasso: g(x) = sum_j lambda_j ||x[jK : (j+1)K]||_2 over the n / K contiguous groups of K = `group`
    elements, 1 <= K <= 64 (no reference class; with SparseMultinomial's layout and K = n_classes a group is a feature's
    row of coefficients).  lambda is a number, or a 1-D array with one entry per GROUP (finite, >= 0; a zero leaves its
    group unpenalised: an intercept row).  `prox` is the specification of the device kernel, operation for operation in
    x's type: the squares of a group are summed by the fixed fold of the power of two KP >= K (zeros behind K, then
    q[:o] + q[o:] for o = KP/2 .. 1), so the result is the device's bit for bit."""

    def __init__(self, lam=1.0, group=1):
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)):
            raise ValueError("the group size must be an integer")
        if not 1 <= group <= 64:
            raise ValueError("the group size must be in 1 .. 64")
        self.group = int(group)
        if np.ndim(lam) == 0:
            if not (np.isfinite(lam) and lam >= 0):
                raise ValueError("parameter λ must be finite and nonnegative")
            self.lam = float(lam)
            return
        lam = np.array(lam, dtype=np.float64)
        if lam.ndim != 1:
            raise ValueError("parameter λ must be a number or a 1-D array (one entry per group)")
        if not np.all(np.isfinite(lam) & (lam >= 0)):
            raise ValueError("parameter λ must have finite, nonnegative entries")
        self.lam = lam

    def _groups(self, x):
        K = self.group
        if x.ndim != 1 or x.shape[0] % K:
            raise ValueError(f"the length of x ({x.shape}) must be a multiple of the group size {K}")
        ng = x.shape[0] // K
        if np.ndim(self.lam) and self.lam.shape[0] != ng:
            raise ValueError(f"λ must have one entry per group ({ng}), not {self.lam.shape[0]}")
        return ng, K

    @staticmethod
    def fold(q):
        """the fixed sum over the last axis (a power of two long): q[:o] + q[o:] for o = KP/2 .. 1"""
        o = q.shape[-1] // 2
        while o >= 1:
            q = q[..., :o] + q[..., o:2 * o]
            o //= 2
        return q[..., 0]

    def __call__(self, x):
        x = np.asarray(x)
        ng, K = self._groups(x)
        return np.sum(self.lam * np.sqrt(np.sum(x.reshape(ng, K) ** 2, axis=1)))

    def prox(self, z, x, gamma):
        T = x.dtype.type
        ng, K = self._groups(x)
        KP = 1
        while KP < K:
            KP *= 2
        vec = np.ndim(self.lam) != 0
        lam = np.asarray(self.lam, dtype=x.dtype) if vec else T(self.lam)
        y = x.reshape(ng, K)
        with np.errstate(all="ignore"):
            q = np.zeros((ng, KP), x.dtype)
            q[:, :K] = y * y
            nrm = np.sqrt(self.fold(q))
            gl = T(gamma) * lam
            zero = nrm <= gl
            big = nrm > gl
            scal = np.where(zero, T(0), np.where(big, T(1) - gl / nrm, nrm - gl)).astype(x.dtype)
            z[...] = np.where(zero[:, None], T(0), scal[:, None] * y).reshape(-1)
            terms = scal * nrm
            if vec:
                return np.sum(lam * terms)
            return lam * np.sum(terms)


class GroupLasso(ProximableFunction):
    """The group Lasso over groups of unequal size, with an optional l1 mix (the sparse-group Lasso):
    g(x) = l1 ||x||_1 + sum_j lambda_j ||x[indptr[j] : indptr[j+1]]||_2 over the contiguous groups a pointer cuts x into
    (indptr[0] = 0, strictly increasing, indptr[-1] = len(x); any size >= 1).  lambda is a number, or a 1-D array with one
    entry per GROUP (finite, >= 0; a zero leaves its group unpenalised: an intercept); l1 is a number, finite and >= 0.  No
    reference class.  `prox` is the specification of the device kernel (k_fbstep_ragged), operation for operation in x's type:
      l1 > 0:  t = gamma * l1 ; u_k = y_k - t where y_k > t, y_k + t where y_k < -t, y_k where it is a NaN, otherwise +0 (the
               ties |y_k| = t included: a zero result is +0 whatever the sign of y_k).  l1 == 0: u = y, not evaluated (-0 stays -0)
      q_k = u_k * u_k ; 64 accumulators a[p] = q[p] + q[p + 64] + q[p + 128] + ... in that order (positions past the group's end
               absent), then NormL21.fold over the 64: a function of the group's size alone.  For a size <= 64 that is NormL21's
               fold over the power of two >= the size (adding +0 to a square is exact), which is how it is evaluated here.
      nrm = sqrt(s) ; gl = gamma * lambda_j ; nrm <= gl: z = 0, scal = 0 ; nrm > gl: scal = 1 - gl / nrm ; otherwise (a NaN)
               scal = nrm - gl ; z_k = scal * u_k
      the value: l1 == 0: NormL21's (sum_j lambda_j (scal nrm), a number lambda times the sum) ; l1 > 0: the sum of
               lambda_j * (scal * nrm) + (l1 * scal) * sabs, sabs the sum of |u_k| in the same accumulator order."""

    def __init__(self, lam=1.0, indptr=(0, 1), l1=0.0):
        p = np.asarray(indptr)
        if p.ndim != 1 or p.shape[0] < 2:
            raise ValueError("indptr must be a 1-D array of at least two entries (one group)")
        if p.dtype == np.bool_ or not np.issubdtype(p.dtype, np.integer):
            raise ValueError("indptr must hold integers")
        p = np.ascontiguousarray(p, dtype=np.int64)
        if p[0] != 0:
            raise ValueError("indptr must start at 0")
        if np.any(np.diff(p) < 1):
            raise ValueError("indptr must be strictly increasing (no empty group)")
        self.indptr = p
        self.ngroups = p.shape[0] - 1
        if isinstance(l1, bool) or np.ndim(l1) != 0 or not (np.isfinite(l1) and l1 >= 0):
            raise ValueError("parameter l1 must be a finite, nonnegative number")
        self.l1 = float(l1)
        if np.ndim(lam) == 0:
            if not (np.isfinite(lam) and lam >= 0):
                raise ValueError("parameter λ must be finite and nonnegative")
            self.lam = float(lam)
            return
        lam = np.array(lam, dtype=np.float64)
        if lam.ndim != 1:
            raise ValueError("parameter λ must be a number or a 1-D array (one entry per group)")
        if not np.all(np.isfinite(lam) & (lam >= 0)):
            raise ValueError("parameter λ must have finite, nonnegative entries")
        if lam.shape[0] != self.ngroups:
            raise ValueError(f"λ must have one entry per group ({self.ngroups}), not {lam.shape[0]}")
        self.lam = lam

    @classmethod
    def from_sizes(cls, lam, sizes, l1=0.0):
        s = np.asarray(sizes)
        if s.ndim != 1 or s.shape[0] < 1 or s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer):
            raise ValueError("sizes must be a 1-D array of integers, one per group")
        return cls(lam, np.concatenate(([0], np.cumsum(s, dtype=np.int64))), l1)

    @property
    def sizes(self):
        return np.diff(self.indptr)

    def _check(self, x):
        if x.ndim != 1 or x.shape[0] != self.indptr[-1]:
            raise ValueError(f"the length of x ({x.shape}) must be indptr[-1] = {self.indptr[-1]}")

    def __call__(self, x):
        x = np.asarray(x)
        self._check(x)
        v = np.sum(self.lam * np.sqrt(np.add.reduceat(x * x, self.indptr[:-1])))
        if self.l1 > 0:
            v = v + self.l1 * np.sum(np.abs(x))
        return v

    def group_sums(self, q):
        """the 64-accumulator sum of every group of q (nonnegative entries or NaNs), bucket by bucket: groups of up to 64 by the
        fold of their power of two, longer ones by their number of 64-element batches"""
        p, size = self.indptr, self.sizes
        s = np.empty(self.ngroups, q.dtype)
        nb = (size + 63) // 64
        kp = np.where(nb == 1, 2 ** np.ceil(np.log2(size)).astype(np.int64), 64)
        for b, w in sorted({(int(b_), int(w_)) for b_, w_ in zip(nb.tolist(), kp.tolist())}):
            G = np.flatnonzero((nb == b) & (kp == w))
            off = np.arange(b * w)
            on = off[None, :] < size[G, None]
            idx = p[G, None] + np.minimum(off[None, :], size[G, None] - 1)
            qq = np.where(on, q[idx], q.dtype.type(0)).reshape(G.shape[0], b, w)
            a = qq[:, 0, :]
            for c in range(1, b):
                a = a + qq[:, c, :]
            s[G] = NormL21.fold(a)
        return s

    def prox(self, z, x, gamma):
        T = x.dtype.type
        self._check(x)
        vec = np.ndim(self.lam) != 0
        lam = np.asarray(self.lam, dtype=x.dtype) if vec else T(self.lam)
        size = self.sizes
        with np.errstate(all="ignore"):
            if self.l1 > 0:
                t = T(gamma) * T(self.l1)
                u = np.where(x > t, x - t, np.where(x < -t, x + t, np.where(np.isnan(x), x, T(0)))).astype(x.dtype)
            else:
                u = x
            nrm = np.sqrt(self.group_sums(u * u))
            gl = T(gamma) * lam
            zero = nrm <= gl
            big = nrm > gl
            scal = np.where(zero, T(0), np.where(big, T(1) - gl / nrm, nrm - gl)).astype(x.dtype)
            z[...] = np.where(np.repeat(zero, size), T(0), np.repeat(scal, size) * u)
            terms = scal * nrm
            if self.l1 > 0:
                sabs = self.group_sums(np.abs(u))
                return np.sum(lam * terms + (T(self.l1) * scal) * sabs)
            if vec:
                return np.sum(lam * terms)
            return lam * np.sum(terms)


class NormL1Nonneg(ProximableFunction):
    """src/proxoperators/normL1Nonneg.jl:9-42"""

    def __init__(self, lam=1.0):
        if lam < 0:
            raise ValueError("λ must be nonnegative")
        self.lam = float(lam)

    def prox(self, z, x, gamma):
        gl = x.dtype.type(gamma * self.lam)
        z[...] = np.where(x >= gl, x - gl, 0)
        return x.dtype.type(self.lam) * np.sum(z)


class NormL1Box(ProximableFunction):
    """src/proxoperators/normL1Box.jl:11-39"""

    def __init__(self, lam=1.0, *, u):
        if lam < 0:
            raise ValueError("parameter λ must be nonnegative")
        self.u = np.ascontiguousarray(u)
        if np.any(self.u < 0):
            raise ValueError("vector u must have nonnegative entries")
        self.lam = float(lam)

    def prox(self, z, x, gamma):
        gl = x.dtype.type(gamma * self.lam)
        z[...] = np.maximum(0, np.minimum(x - gl, self.u))
        return x.dtype.type(self.lam) * np.sum(z)


class NormL0Box(ProximableFunction):
    """src/proxoperators/normL0Box.jl:12-58: lambda*nnz(x) + indicator of [0, u]."""

    def __init__(self, lam=1.0, *, u):
        if lam < 0:
            raise ValueError("parameter λ must be nonnegative")
        self.u = np.ascontiguousarray(u)
        if np.any(self.u < 0):
            raise ValueError("vector u must have nonnegative entries")
        self.lam = float(lam)


class NormLpPowerNonneg(ProximableFunction):
    """src/proxoperators/normLpNonneg.jl:14-40: alpha * sum x^p on x >= 0, 0 < p < 1."""

    def __init__(self, p, *, alpha=1.0):
        if p <= 0:
            raise ValueError("p must be positive")
        if p >= 1:
            raise ValueError("p must be smaller than one")
        if alpha < 0:
            raise ValueError("alpha must be nonnegative")
        self.p, self.alpha = float(p), float(alpha)


class NormLpPowerBox(ProximableFunction):
    """src/proxoperators/normLpBox.jl:11-45: alpha * sum x^p on 0 <= x <= u, 0 < p < 1."""

    def __init__(self, p, alpha=1.0, *, u):
        if p <= 0:
            raise ValueError("p must be positive")
        if p >= 1:
            raise ValueError("p must be smaller than one")
        if alpha < 0:
            raise ValueError("alpha must be nonnegative")
        self.u = np.ascontiguousarray(u)
        if np.any(self.u < 0):
            raise ValueError("vector u must have nonnegative entries")
        self.p, self.alpha = float(p), float(alpha)


class IndBox(ProximableFunction):
    """ProximalOperators.IndBox(lb, ub) (test_nonconvex_qp.jl:15); scalar or vector bounds."""

    def __init__(self, lb, ub):
        self.lb = lb
        self.ub = ub
        if np.any(np.asarray(lb) > np.asarray(ub)):
            raise ValueError("bounds must satisfy lb <= ub")

    def prox(self, z, x, gamma=1.0):
        z[...] = np.where(x < self.lb, self.lb, np.where(x > self.ub, self.ub, x))
        return x.dtype.type(0)


# ------------------------------------------------------------------------- c
class IdentityFunction(SmoothFunction):
    """test/definitions/identityFunction.jl:3-13"""

    def eval(self, cx, x):
        cx[...] = x

    def jtprod(self, jtv, x, v):
        jtv[...] = v


class DenseAffine(SmoothFunction):
    """c(x) = A x - b with a dense row-major A[ny][n]: `ConstraintBasisPursuit`
    (demo/basispursuit.jl:38-49); eval! = A*x - b, jtprod! = A'*v."""

    def __init__(self, A, b):
        self.A = np.ascontiguousarray(A)
        self.b = np.ascontiguousarray(b)
        if self.A.ndim != 2 or self.b.shape != (self.A.shape[0],):
            raise ValueError("A must be ny-by-n and b of length ny")

    def eval(self, cx, x):
        cx[...] = self.A @ x - self.b

    def jtprod(self, jtv, x, v):
        jtv[...] = self.A.T @ v


class SparseAffine(_CSR, SmoothFunction):
    """c(x) = A x - b with A[ny][n] in CSR (indptr[ny + 1], indices[nnz] 0-based, data[nnz]): the structured, never
    densified constraint map of demo/obstacle.jl:93-113 (c(x) = x1 + T x2 - x3).  The column indices of a row need not
    be sorted, an index that occurs twice in a row contributes twice, an empty row gives -b_i and an empty column a
    zero of A'v.  eval! / jtprod! below are numpy (the host outer loop, and the generic-oracle protocol); on the device
    the kind is BZ_C_SPARSE_AFFINE."""

    def __init__(self, indptr, indices, data, b, n):
        self.b = np.ascontiguousarray(b)
        self.n = int(n)
        self._csr_types(indptr, indices, data, self.b, "b", both=True)
        self.ny = self.b.shape[0]
        if self.n <= 0 or self.n > _I32_MAX or self.ny <= 0:
            raise ValueError("n must be in 1 .. 2^31 - 1 and b non-empty")
        self._csr_shape(self.ny, self.n, "ny")

    @classmethod
    def from_dense(cls, A, b):
        csr, n = cls._csr_of_dense(A, "A must be ny-by-n")
        return cls(*csr, b, n)

    @classmethod
    def from_scipy(cls, M, b):
        csr, n = cls._csr_of_scipy(M)
        return cls(*csr, b, n)

    def eval(self, cx, x):
        cx[...] = self._matvec(x) - self.b

    def jtprod(self, jtv, x, v):
        jtv[...] = self._rmatvec(v)


# ------------------------------------------------------------------------- D
class ZeroSet(ClosedSetBase):
    """src/projections/zeroSet.jl:8-20"""

    def proj(self, s, v):
        s[...] = 0


class FreeSet(ClosedSetBase):
    """src/projections/freeSet.jl:8-20"""

    def proj(self, s, v):
        s[...] = v


class IndicatorSet(ClosedSetBase):
    """src/projections/indicatorSet.jl:4-11"""

    def __init__(self, f):
        self.f = f

    def proj(self, s, v):
        self.f.prox(s, v, 1.0)


def ClosedSet(f):
    """src/Bazinga.jl:18"""
    return IndicatorSet(f)


class PairwiseSet(ClosedSetBase):
    """D = product of a 2-element set over the ADJACENT pairs (c(x)[2j], c(x)[2j+1]) — how demo/mpvca.jl:
    105-106,147-148 and demo/eitheror.jl:79-88,123-130 build their sets from the package's 2-element
    projections.  kind: "vc" (project_onto_VC_set!, vanishingConstraints.jl:27-46), "cc"
    (project_onto_CC_set!, complementarityConstraints.jl:8-20), "eitheror" / "xor"
    (orConstraints.jl:7-17 / 24-36)."""
    KINDS = ("vc", "cc", "eitheror", "xor")

    def __init__(self, kind, layout="adjacent"):
        """layout="adjacent": pairs (c(x)[2j], c(x)[2j+1]); layout="split": pairs (c(x)[i], c(x)[i+N]), N = ny/2, the way
        demo/obstacle.jl:151-168 (SetObstacleRed) lays its complementarity pairs out.  The device kernels work on
        adjacent pairs (a pair is one 16-byte pack); the split layout is the same problem under the interleaving
        permutation, which the host binding applies to every vector at the boundary (device.Problem)."""
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {self.KINDS}")
        if layout not in ("adjacent", "split"):
            raise ValueError("layout must be 'adjacent' or 'split'")
        self.kind = kind
        self.layout = layout

    def proj(self, s, v):
        """the 2-element projections over adjacent pairs (host protocol: only used when another oracle of the
        problem is generic)"""
        if self.layout == "split":
            N = v.shape[0] // 2
            x1, x2 = v[:N], v[N:]
        else:
            x1, x2 = v[0::2], v[1::2]
        z1, z2 = x1.copy(), x2.copy()
        if self.kind == "vc":          # vanishingConstraints.jl:27-46
            a = x1 <= 0
            b = ~a & (x2 >= 0)
            c = ~a & ~b & (x1 + x2 > 0)
            z1[...] = np.where(b | c, x1, 0)
            z2[...] = np.where(a | b | ~c, x2, 0)
            z2[c] = 0
        elif self.kind == "cc":        # complementarityConstraints.jl:8-20
            both = (x1 > 0) & (x2 > 0)
            z1[...] = np.where(both, np.where(x2 > x1, 0, x1), np.maximum(x1, 0))
            z2[...] = np.where(both, np.where(x2 > x1, x2, 0), np.maximum(x2, 0))
        elif self.kind == "eitheror":  # orConstraints.jl:7-17
            both = (x1 < 0) & (x2 < 0)
            z1[...] = np.where(both & (x1 > x2), 0, x1)
            z2[...] = np.where(both & ~(x1 > x2), 0, x2)
        else:                          # xor, orConstraints.jl:24-36
            same = x1 * x2 > 0
            up = x1 > x2
            z1[...] = np.where(same, np.where(up, np.maximum(x1, 0), np.minimum(x1, 0)), x1)
            z2[...] = np.where(same, np.where(up, np.minimum(x2, 0), np.maximum(x2, 0)), x2)
        if self.layout == "split":
            s[:N], s[N:] = z1, z2
        else:
            s[0::2] = z1
            s[1::2] = z2


def VanishingConstraintPairs():
    return PairwiseSet("vc")


def ComplementarityPairs():
    return PairwiseSet("cc")


def EitherOrPairs():
    return PairwiseSet("eitheror")


def XorPairs():
    return PairwiseSet("xor")


# ------------------------------------------------------------------ lowering
def split_permutation(n):
    """perm with x_adjacent = x_split[perm]: position 2j holds element j, position 2j+1 element j + N (N = n/2)"""
    N = n // 2
    perm = np.empty(n, np.int64)
    perm[0::2] = np.arange(N)
    perm[1::2] = np.arange(N) + N
    return perm


def _vec(a, dtype, n, name):
    v = np.ascontiguousarray(a, dtype=dtype)
    if v.shape != (n,):
        raise ValueError(f"{name} must have length {n}")
    return v


# the f kinds that carry a CSR matrix: class -> (kind, what a wrong column count raises, the name of the vector in f_b)
_SPARSE_F = {
    SparseQuadratic: (L.BZ_F_SPARSE_QUADRATIC, "Q must be {n}-by-{n}", "q"),
    SparseLeastSquares: (L.BZ_F_SPARSE_LEAST_SQUARES, "A must have {n} columns", "b"),
    SparseLogistic: (L.BZ_F_SPARSE_LOGISTIC, "A must have {n} columns", "labels"),
    SparseGLM: (L.BZ_F_SPARSE_GLM, "A must have {n} columns", "b"),
    SparseMultinomial: (L.BZ_F_SPARSE_MULTINOMIAL, "x must have n_features * n_classes = {fn} elements, not {n}", "labels"),
    SparseMultiGLM: (L.BZ_F_SPARSE_MULTI_GLM, "x must have n_features * K = {fn} elements, not {n}", "B"),
}

_LOWERED_F = lambda f: isinstance(f, (Zero, DiagQuadratic, LeastSquares, Quadratic, *_SPARSE_F, Stencil5ptQuadratic))
_LOWERED_G = lambda g: isinstance(g, (Zero, IndFree, NormL1, ElasticNet, NormL21, GroupLasso, NormL1Nonneg, NormL1Box, NormL0Box, NormLpPowerNonneg,
                                      NormLpPowerBox, IndBox))
_LOWERED_C = lambda c: isinstance(c, (IdentityFunction, DenseAffine, SparseAffine))
_LOWERED_D = lambda D: isinstance(D, (ZeroSet, FreeSet, PairwiseSet)) or \
    (isinstance(D, IndicatorSet) and isinstance(D.f, (IndBox, IndFree)))


class CallbackError(RuntimeError):
    """An oracle callback raised: the original exception is the __cause__."""


def lower_generic(f, g, c, D, n, ny, dtype, slack=False):
    """Generic oracles -> host callbacks (BZ_*_CALLBACK).  Returns (desc, keep): `keep` holds the ctypes thunks and
    must live as long as the problem; keep[-1] is the list exceptions raised inside callbacks are parked in."""
    if slack:
        raise UnsupportedOracle("generic (callback) oracles are not available in the slack (ALS) form")
    for obj, names, what in ((f, ("gradient",), "f"), (g, ("prox",), "g"), (c, ("eval", "jtprod"), "c"), (D, ("proj",), "D")):
        for nm in names:
            if not callable(getattr(obj, nm, None)):
                raise UnsupportedOracle(f"{what} of type {type(obj).__name__} is neither a lowered oracle type nor a generic "
                                        f"one (no `{nm}` method)")
    dt = np.dtype(dtype)
    errors = []

    ctype = C.c_double if dt == np.float64 else C.c_float

    def arr(ptr, cnt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(cnt,))

    def guard(fn, default):
        def wrapped(*a):
            if errors:                      # an earlier callback of this library call failed: evaluate nothing more
                L.load().bz_callback_abort()
                return default
            try:
                return fn(*a)
            except BaseException as e:      # noqa: BLE001  (nothing may unwind through the C frames)
                errors.append(e)
                # the library call in progress ends with BZ_ERR_CALLBACK as soon as this callback has returned
                # (device.Problem._call then raises CallbackError from the parked exception)
                L.load().bz_callback_abort()
                return default
        return wrapped

    def f_gradient(_u, px, pdfx, nn):
        return float(f.gradient(arr(pdfx, nn), arr(px, nn)))

    def g_prox(_u, px, gamma, pz, nn):
        return float(g.prox(arr(pz, nn), arr(px, nn), dt.type(gamma)))

    def c_eval(_u, px, pcx, nn, nny):
        c.eval(arr(pcx, nny), arr(px, nn))

    def c_jtprod(_u, px, pv, pjtv, nn, nny):
        c.jtprod(arr(pjtv, nn), arr(px, nn), arr(pv, nny))

    def d_proj(_u, pv, ps, nny):
        D.proj(arr(ps, nny), arr(pv, nny))

    d = L.ProblemDesc()
    d.dtype = L.BZ_F64 if dt == np.float64 else L.BZ_F32
    d.n, d.ny, d.slack = n, ny, 0
    d.f_kind, d.g_kind, d.c_kind, d.D_kind = L.BZ_F_CALLBACK, L.BZ_G_CALLBACK, L.BZ_C_CALLBACK, L.BZ_D_CALLBACK
    nan = float("nan")
    thunks = [L.F_GRADIENT_FN(guard(f_gradient, nan)), L.G_PROX_FN(guard(g_prox, nan)), L.C_EVAL_FN(guard(c_eval, None)),
              L.C_JTPROD_FN(guard(c_jtprod, None)), L.D_PROJ_FN(guard(d_proj, None))]
    d.cb_f_gradient, d.cb_g_prox, d.cb_c_eval, d.cb_c_jtprod, d.cb_D_proj = thunks
    return d, [f, g, c, D, thunks, errors]


def lower(f, g, c, D, n, ny, dtype, slack=False):
    """(f, g, c, D) -> (ProblemDesc, keepalive list).  Raises UnsupportedOracle.
    slack=True: the ALS form on xs = [x; s] (src/utilities/auglagfunslack.jl)."""
    dtype = np.dtype(dtype)
    if dtype in (np.float64, np.float32) and not (_LOWERED_F(f) and _LOWERED_G(g) and _LOWERED_C(c) and _LOWERED_D(D)):
        return lower_generic(f, g, c, D, n, ny, dtype, slack)
    if dtype == np.float64:
        code = L.BZ_F64
    elif dtype == np.float32:
        code = L.BZ_F32
    else:
        raise UnsupportedOracle(f"eltype {dtype} is not lowered (Float64/Float32 only)")
    d = L.ProblemDesc()
    keep = []
    d.dtype, d.n, d.ny = code, n, ny
    d.slack = 1 if slack else 0
    # split-layout pairwise set: every per-element parameter vector goes to the device in the interleaved
    # (adjacent-pair) order; device.Problem permutes the state vectors at the boundary with the same map
    perm = split_permutation(n) if (isinstance(D, PairwiseSet) and D.layout == "split") else None
    if perm is not None and not isinstance(f, (Zero, DiagQuadratic)):
        raise UnsupportedOracle("split-layout pairwise sets are lowered with an element-wise f (Zero, DiagQuadratic)")

    def ptr(a):
        if perm is not None and a.ndim == 1 and a.shape[0] == n:
            a = np.ascontiguousarray(a[perm])
        keep.append(a)
        return a.ctypes.data

    def csr(side, a):
        """the matrix of a (_CSR) in the four <side>_sp_* fields"""
        setattr(d, side + "_sp_rowptr", ptr(a.indptr))
        setattr(d, side + "_sp_col", ptr(a.indices))
        setattr(d, side + "_sp_val", ptr(np.ascontiguousarray(a.data, dtype=dtype)))
        setattr(d, side + "_sp_nnz", a.nnz)

    def num_or_vec(field, value, cnt, name):
        """a number in d.<field>, or a vector of cnt elements behind d.<field>_vec"""
        if np.ndim(value) == 0:
            setattr(d, field, float(value))
        else:
            setattr(d, field + "_vec", ptr(_vec(value, dtype, cnt, name)))

    def sparse_f(cls, kind, columns, name):
        """any f with a CSR matrix (a row of _SPARSE_F)"""
        # what the library refuses with these kinds, refused here before any device call
        if slack:
            raise UnsupportedOracle(f"{cls.__name__} is not lowered in the slack (ALS) form")
        if isinstance(c, DenseAffine):
            raise UnsupportedOracle(f"{cls.__name__} is not lowered beside a dense c (DenseAffine)")
        if f.n != n:
            raise ValueError(columns.format(n=n, fn=f.n))
        d.f_kind = kind
        csr("f", f)
        if cls is SparseQuadratic:                       # (n-by-n: f_rows stays 0, and f_b carries q)
            d.f_b = ptr(_vec(f.q, dtype, n, name))
            return
        d.f_rows = f.m
        d.f_b = ptr(_vec(f.b, dtype, f.m * (f.n_classes if cls is SparseMultiGLM else 1), name))     # (B: m rows of K, row-major)
        delta, finite = None, "scale and scale * weights"          # what must be finite in dtype
        if cls in (SparseGLM, SparseMultiGLM):
            d.f_loss = SparseGLM.LOSSES.index(f.loss)
            d.f_loss_delta = 0.0 if f.delta is None else f.delta
            delta, finite = f.delta, "scale, scale * weights and delta"
        if cls in (SparseMultinomial, SparseMultiGLM):
            d.f_classes = f.n_classes
        if isinstance(f, _RowWeighted):
            d.f_scale = f.scale
            if not np.all(np.isfinite(f.row_weights(dtype))) or (delta is not None and not np.isfinite(dtype.type(delta))):
                raise ValueError(f"{finite} must be finite in {dtype}")
            if f.weights is not None:
                d.f_w = ptr(_vec(f.weights, dtype, f.m, "weights"))

    # f
    if isinstance(f, Zero):
        d.f_kind = L.BZ_F_ZERO
    elif isinstance(f, DiagQuadratic):
        d.f_kind = L.BZ_F_DIAG_QUADRATIC
        d.f_q = ptr(_vec(f.q, dtype, n, "q"))
        d.f_b = ptr(_vec(f.b, dtype, n, "b"))
    elif isinstance(f, LeastSquares):
        d.f_kind = L.BZ_F_LEAST_SQUARES
        if f.A.shape[1] != n:
            raise ValueError(f"A must have {n} columns")
        d.f_A = ptr(np.ascontiguousarray(f.A, dtype=dtype))
        d.f_rows = f.A.shape[0]
        d.f_b = ptr(_vec(f.b, dtype, f.A.shape[0], "b"))
    elif isinstance(f, Quadratic):
        d.f_kind = L.BZ_F_QUADRATIC
        if f.Q.shape != (n, n):
            raise ValueError(f"Q must be {n}-by-{n}")
        d.f_A = ptr(np.ascontiguousarray(f.Q, dtype=dtype))
        d.f_rows = n
        d.f_b = ptr(_vec(f.q, dtype, n, "q"))
    elif isinstance(f, tuple(_SPARSE_F)):
        sparse_f(*next((cls, *row) for cls, row in _SPARSE_F.items() if isinstance(f, cls)))
    elif isinstance(f, Stencil5ptQuadratic):
        d.f_kind = L.BZ_F_STENCIL5
        d.f_grid_nx, d.f_grid_ny = f.nx, f.ny
        d.f_b = ptr(_vec(f.b, dtype, n, "b"))
    else:
        raise UnsupportedOracle(f"f of type {type(f).__name__} is not lowered to the device")
    # g
    if isinstance(g, (Zero, IndFree)):
        d.g_kind = L.BZ_G_ZERO
    elif isinstance(g, NormL1):
        d.g_kind = L.BZ_G_NORM_L1
        num_or_vec("g_lambda", g.lam, n, "λ")
    elif isinstance(g, ElasticNet):
        g._check(dtype)
        d.g_kind, d.g_lambda, d.g_l2 = L.BZ_G_ELASTIC_NET, g.l1, g.l2
        if g.weights is not None:
            d.g_weights = ptr(_vec(g.weights, dtype, n, "weights"))
    elif isinstance(g, NormL21):
        # what the library refuses with this kind, refused here before any device call
        if slack:
            raise UnsupportedOracle("NormL21 is not lowered in the slack (ALS) form")
        if perm is not None:
            raise UnsupportedOracle("NormL21 is not lowered beside a split-layout pairwise set (the groups would be permuted)")
        if n % g.group:
            raise ValueError(f"n = {n} must be a multiple of the group size {g.group}")
        d.g_kind, d.g_group = L.BZ_G_NORM_L21, g.group
        num_or_vec("g_lambda", g.lam, n // g.group, "λ")
    elif isinstance(g, GroupLasso):
        # what the library refuses with this kind, refused here before any device call
        if slack:
            raise UnsupportedOracle("GroupLasso is not lowered in the slack (ALS) form")
        if perm is not None:
            raise UnsupportedOracle("GroupLasso is not lowered beside a split-layout pairwise set (the groups would be permuted)")
        if g.indptr[-1] != n:
            raise ValueError(f"indptr[-1] = {g.indptr[-1]} must be n = {n}")
        d.g_kind, d.g_ngroups, d.g_l1 = L.BZ_G_GROUP_LASSO, g.ngroups, g.l1
        d.g_group_ptr = ptr(g.indptr)
        num_or_vec("g_lambda", g.lam, g.ngroups, "λ")
    elif isinstance(g, NormL1Nonneg):
        d.g_kind, d.g_lambda = L.BZ_G_NORM_L1_NONNEG, g.lam
    elif isinstance(g, NormL1Box):
        d.g_kind, d.g_lambda = L.BZ_G_NORM_L1_BOX, g.lam
        d.g_u = ptr(_vec(g.u, dtype, n, "u"))
    elif isinstance(g, NormL0Box):
        d.g_kind, d.g_lambda = L.BZ_G_NORM_L0_BOX, g.lam
        d.g_u = ptr(_vec(g.u, dtype, n, "u"))
    elif isinstance(g, NormLpPowerNonneg):
        d.g_kind, d.g_lambda, d.g_p = L.BZ_G_NORM_LP_NONNEG, g.alpha, g.p
    elif isinstance(g, NormLpPowerBox):
        d.g_kind, d.g_lambda, d.g_p = L.BZ_G_NORM_LP_BOX, g.alpha, g.p
        d.g_u = ptr(_vec(g.u, dtype, n, "u"))
    elif isinstance(g, IndBox):
        d.g_kind = L.BZ_G_IND_BOX
        num_or_vec("g_lo", g.lb, n, "lb")
        num_or_vec("g_hi", g.ub, n, "ub")
    else:
        raise UnsupportedOracle(f"g of type {type(g).__name__} is not lowered to the device")
    # c
    if isinstance(c, IdentityFunction):
        d.c_kind = L.BZ_C_IDENTITY
        if ny != n:
            raise ValueError("IdentityFunction requires length(y0) == length(x0)")
    elif isinstance(c, DenseAffine):
        d.c_kind = L.BZ_C_DENSE_AFFINE
        if c.A.shape != (ny, n):
            raise ValueError(f"A must be {ny}-by-{n}")
        A = np.ascontiguousarray(c.A, dtype=dtype)
        d.c_A = ptr(A)
        d.c_b = ptr(_vec(c.b, dtype, ny, "b"))
    elif isinstance(c, SparseAffine):
        # what the library refuses with this kind, refused here before any device call
        if slack:
            raise UnsupportedOracle("SparseAffine is not lowered in the slack (ALS) form")
        if not isinstance(f, (Zero, DiagQuadratic, *_SPARSE_F)):
            raise UnsupportedOracle(f"SparseAffine is lowered with an element-wise f (Zero, DiagQuadratic), not {type(f).__name__}")
        if isinstance(D, PairwiseSet):
            raise UnsupportedOracle("pairwise D sets need c = IdentityFunction")
        if (c.ny, c.n) != (ny, n):
            raise ValueError(f"A must be {ny}-by-{n}")
        d.c_kind = L.BZ_C_SPARSE_AFFINE
        csr("c", c)
        d.c_b = ptr(_vec(c.b, dtype, ny, "b"))
    else:
        raise UnsupportedOracle(f"c of type {type(c).__name__} is not lowered to the device")
    # D
    if isinstance(D, ZeroSet):
        d.D_kind = L.BZ_D_ZERO
    elif isinstance(D, FreeSet):
        d.D_kind = L.BZ_D_FREE
    elif isinstance(D, IndicatorSet) and isinstance(D.f, IndBox):
        d.D_kind = L.BZ_D_BOX
        num_or_vec("D_lo", D.f.lb, ny, "lb")
        num_or_vec("D_hi", D.f.ub, ny, "ub")
    elif isinstance(D, IndicatorSet) and isinstance(D.f, IndFree):
        d.D_kind = L.BZ_D_FREE
    elif isinstance(D, PairwiseSet):
        d.D_kind = {"vc": L.BZ_D_VC_PAIRS, "cc": L.BZ_D_CC_PAIRS, "eitheror": L.BZ_D_EITHEROR_PAIRS,
                    "xor": L.BZ_D_XOR_PAIRS}[D.kind]
        if ny % 2:
            raise ValueError("pairwise sets need an even number of constraints")
    else:
        raise UnsupportedOracle(f"D of type {type(D).__name__} is not lowered to the device")
    return d, keep
