"""The numpy restatement of masked coordinate descent (include/smallk_amd.h: smk_nmf_masked_device): NMF fitted to the
stored entries of a sparse matrix only, from CSC arrays.  Orientation, penalties and stopping rule are cd_reference.py's.

A sweep updates X (k x N) against G (k x M, the factor whose rows the entries name) over one CSC (indptr over the N columns, row
indices in [0, M), values): per column j, with r_e = a_e - G[:, i_e] . x_j kept current, for t = 0 .. k-1 in order
    grad = -sum_e G[t, i_e] r_e + l1 + l2 x[t];  hess = sum_e G[t, i_e]^2 + l2;  violation += |x[t] == 0 ? min(0, grad) : grad|
    unless hess == 0: xn = max(x[t] - grad / hess, 0);  r_e -= G[t, i_e] (xn - x[t]);  x[t] = xn
All columns advance together, one t at a time.  Two summation orders of the two sums per step ("seq": numpy.bincount, the entries of
a column one after the other in storage order; "pair": numpy.add.reduceat, numpy's blocked pairwise order) and numpy.longdouble
(with "pair"; bincount adds in double) are available, so that the tests can tell what hangs on rounding.
"""
import numpy as np


def transpose_csc(data, indices, indptr, shape):
    """the CSC of A' with the entries of a row in column order (a stable sort by row)"""
    m, n = shape
    col = np.repeat(np.arange(n), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=m))]).astype(np.int64)
    return data[order], col[order], ptr, (n, m)


class Csc:
    """one CSC with what the sweep needs of it"""

    def __init__(self, data, indices, indptr, shape):
        self.data = np.asarray(data, dtype=np.float64)
        self.rows = np.asarray(indices).astype(np.int64)
        self.ptr = np.asarray(indptr).astype(np.int64)
        self.shape = (int(shape[0]), int(shape[1]))
        self.col = np.repeat(np.arange(self.shape[1]), np.diff(self.ptr))
        self.live = np.nonzero(np.diff(self.ptr) > 0)[0]          # the columns that store something
        self.starts = self.ptr[self.live]

    def column_sums(self, v, order):
        """sum of v over the entries of each column"""
        N = self.shape[1]
        if order == "seq":
            if v.dtype != np.float64:
                raise ValueError("the seq order adds in double")
            return np.bincount(self.col, weights=v, minlength=N)
        out = np.zeros(N, dtype=v.dtype)
        if self.live.size:
            out[self.live] = np.add.reduceat(v, self.starts)
        return out


def residuals(X, G, csc):
    """a - G[:, i] . x_j per stored entry, the products added for t = 0 .. k-1 in order"""
    dt = X.dtype
    acc = np.zeros(csc.data.shape[0], dtype=dt)
    for t in range(X.shape[0]):
        acc += G[t, csc.rows] * X[t, csc.col]
    return csc.data.astype(dt) - acc


def sweep(X, G, csc, l1, l2, *, order="seq"):
    """in place on X (k x N, float64 or longdouble); returns the violation"""
    k, N = X.shape
    dt = X.dtype
    l1, l2 = dt.type(l1), dt.type(l2)
    G = np.asarray(G, dtype=dt)
    r = residuals(X, G, csc)
    viol = dt.type(0)
    for t in range(k):
        w = G[t, csc.rows]
        xt = X[t].copy()
        grad = (l1 - csc.column_sums(w * r, order)) + l2 * xt
        hess = csc.column_sums(w * w, order) + l2
        pg = np.where(xt == 0, np.minimum(grad, 0), grad)
        viol += np.abs(pg).sum()
        move = hess != 0
        xn = np.where(move, np.maximum(xt - grad / np.where(move, hess, 1), 0), xt)
        r -= w * (xn - xt)[csc.col]
        X[t] = xn
    return viol


def fit(csc_tuple, W0, H0, *, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, order="seq", dtype=np.float64,
        after_first=None):
    """the loop of smk_nmf_masked_device; returns a dict: W, H, n_iter, converged, violation_init, violation, error, ratios.
    after_first: called with (Wt, H) after iteration 1 (the single sweeps of the tests)"""
    dt = np.dtype(dtype)
    data, indices, indptr, shape = csc_tuple
    m, n = shape
    A = Csc(data, indices, indptr, shape)
    At = Csc(*transpose_csc(A.data, A.rows, A.ptr, A.shape))
    Wt = np.array(np.asarray(W0, dtype=dt).T, order="C")
    H = np.array(H0, dtype=dt, order="C")
    l1h, l2h = m * alpha_H * l1_ratio, m * alpha_H * (1.0 - l1_ratio)
    l1w, l2w = n * alpha_W * l1_ratio, n * alpha_W * (1.0 - l1_ratio)
    ratios, v0, v, converged, it = [], None, None, False, 0
    for it in range(1, max_iter + 1):
        v = sweep(H, Wt, A, l1h, l2h, order=order)
        if update_W:
            v = v + sweep(Wt, H, At, l1w, l2w, order=order)
        if it == 1:
            v0 = v
            if after_first is not None:
                after_first(Wt, H)
        ratios.append(float(v / v0) if v0 != 0 else 0.0)
        if v0 == 0 or v / v0 <= tol:
            converged = True
            break
    err = np.sqrt((residuals(H, Wt, A) ** 2).sum())
    return {"W": np.asarray(Wt.T, dtype=np.float64), "H": np.asarray(H, dtype=np.float64), "n_iter": it, "converged": converged,
            "violation_init": float(v0), "violation": float(v), "error": float(err), "ratios": ratios}


def masked_residual(csc_tuple, W, H, dtype=np.longdouble):
    """(sum (a - w_i . h_j)^2, sum a^2, count, the first two per column, sum |terms| of the first) over the stored entries"""
    A = Csc(*csc_tuple)
    dt = np.dtype(dtype)
    r = residuals(np.asarray(H, dtype=dt), np.array(np.asarray(W, dtype=dt).T, order="C"), A)
    a = A.data.astype(dt)
    N = A.shape[1]
    col_r, col_a = np.zeros(N, dtype=dt), np.zeros(N, dtype=dt)
    np.add.at(col_r, A.col, r * r)
    np.add.at(col_a, A.col, a * a)
    absdot = np.zeros(a.shape[0], dtype=dt)                 # the size of the terms a residual is formed from
    Wt = np.asarray(W, dtype=dt).T
    for t in range(Wt.shape[0]):
        absdot += np.abs(Wt[t, A.rows] * np.asarray(H, dtype=dt)[t, A.col])
    terms = (np.abs(a) + absdot) ** 2
    col_terms = np.zeros(N, dtype=dt)
    np.add.at(col_terms, A.col, terms)
    return float((r * r).sum()), float((a * a).sum()), int(a.shape[0]), col_r.astype(np.float64), col_a.astype(np.float64), float(terms.sum()), col_terms.astype(np.float64)
