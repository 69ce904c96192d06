"""The numpy restatement of weighted masked beta-divergence NMF on a dense matrix (include/smallk_amd.h:
smk_nmf_weighted_dense_device) in a float type of the caller's choice: tests/masked_dense_reference.py's update,
divergence and loop for beta = 2, 1, 0 with the weight of each entry inside every sum over entries.  A NaN in A is "not measured"
whatever its weight; no penalties."""
import numpy as np

from masked_dense_reference import EPS, EPS64


def sums(A, V, R, X, beta):
    """(numerator, denominator) of the update of X (k x cols), before the 0 -> EPS rule; A, V rows x cols, R rows x k"""
    miss, zero = np.isnan(A), X.dtype.type(0)
    a, w, d = np.where(miss, zero, A), np.where(miss, zero, V), R @ X
    if beta == 2:
        qn, qd = a, d
    else:
        d[d < EPS] = EPS
        r = 1 / d
        qn, qd = (a / d, np.ones_like(d)) if beta == 1 else ((r * r) * a, r)
    return R.T @ (w * qn), R.T @ (w * qd)


def _update(A, V, R, X, beta, flush):
    num, den = sums(A, V, R, X, beta)
    den[den == 0] = EPS
    num /= den
    X *= np.sqrt(num) if beta == 0 else num
    if flush:
        X[X < EPS64] = 0.0
    return X


def step_h(A, V, W, H, beta):
    """in place on H (k x n)"""
    return _update(np.asarray(A, dtype=H.dtype), np.asarray(V, dtype=H.dtype), W, H, beta, beta < 1)


def step_w(A, V, W, H, beta):
    """in place on W (m x k), with the new H"""
    Wt, T = np.ascontiguousarray(W.T), lambda M: np.ascontiguousarray(np.asarray(M, dtype=W.dtype).T)
    _update(T(A), T(V), np.ascontiguousarray(H.T), Wt, beta, beta <= 1)
    W[...] = Wt.T
    return W


def divergence(A, V, W, H, beta):
    """(D_w over the measured entries, not clamped; the sum of the absolute values of its terms; the sum of the weights of the
    measured entries)"""
    A, V = np.asarray(A, dtype=W.dtype), np.asarray(V, dtype=W.dtype)
    meas = ~np.isnan(A)
    a, w, d = A[meas], V[meas], (W @ H)[meas]
    if beta == 2:
        t = w * (a - d) ** 2
        return t.sum() / 2, t.sum() / 2, w.sum()
    big = a > EPS
    q = a[big] / np.maximum(d[big], EPS)
    if beta == 1:
        t = w[big] * a[big] * np.log(q)
        return t.sum() - (w * a).sum() + (w * d).sum(), np.abs(t).sum() + (w * a).sum() + (w * d).sum(), w.sum()
    t = w[big] * np.log(q)
    return (w[big] * q).sum() - w.sum() - t.sum(), (w[big] * q).sum() + w.sum() + np.abs(t).sum(), w.sum()


def fit(A, V, W0, H0, *, beta, max_iter, dtype=np.float64):
    """max_iter iterations of smk_nmf_weighted_dense_device with tol = 0; returns a dict: W, H, error"""
    A, V = np.asarray(A, dtype=dtype), np.asarray(V, dtype=dtype)
    W, H = np.array(W0, dtype=dtype), np.array(H0, dtype=dtype)
    for _ in range(max_iter):
        step_h(A, V, W, H, beta)
        step_w(A, V, W, H, beta)
    return {"W": np.asarray(W, dtype=np.float64), "H": np.asarray(H, dtype=np.float64),
            "error": float(np.sqrt(2 * max(divergence(A, V, W, H, beta)[0], 0)))}
