"""The numpy restatement of masked beta-divergence NMF on a dense matrix (include/smallk_amd.h: smk_nmf_masked_dense_device;
DESIGN.md 24) in a float type of the caller's choice: tests/beta_reference.py's iteration for beta = 2, 1, 0 with every sum over
entries restricted to the measured ones.  A NaN in A is "not measured"; the masks are np.isnan(A), the sums np.where products."""
import numpy as np

EPS, EPS64, U53, FIT_BAR = 2.0 ** -23, 2.0 ** -52, 2.0 ** -53, 1e-12


def _update(A, R, X, beta, l1, l2, flush):
    """one half-iteration in place on X (k x cols); A rows x cols, R rows x k the factor of A's rows"""
    miss, zero = np.isnan(A), X.dtype.type(0)
    a, d = np.where(miss, zero, A), R @ X
    if beta == 2:
        qn, qd = a, np.where(miss, zero, d)
    else:
        d[d < EPS] = EPS
        r = 1 / d
        qn, qd = (a / d, np.where(miss, zero, X.dtype.type(1))) if beta == 1 else ((r * r) * a, np.where(miss, zero, r))
    num, den = R.T @ qn, R.T @ qd
    if l1 > 0:
        den += X.dtype.type(l1)
    if l2 > 0:
        den = den + X.dtype.type(l2) * X
    den[den == 0] = EPS
    num /= den
    X *= np.sqrt(num) if beta == 0 else num
    if flush:
        X[X < EPS64] = 0.0
    return X


def step_h(A, W, H, beta, l1=0.0, l2=0.0):
    """in place on H (k x n)"""
    return _update(np.asarray(A, dtype=H.dtype), W, H, beta, l1, l2, beta < 1)


def step_w(A, W, H, beta, l1=0.0, l2=0.0):
    """in place on W (m x k), with the new H"""
    Wt = np.ascontiguousarray(W.T)
    _update(np.ascontiguousarray(np.asarray(A, dtype=W.dtype).T), np.ascontiguousarray(H.T), Wt, beta, l1, l2, beta <= 1)
    W[...] = Wt.T
    return W


def divergence(A, W, H, beta):
    """(D over the measured entries, not clamped; the sum of the absolute values of its terms; the number of measured entries)"""
    A = np.asarray(A, dtype=W.dtype)
    meas = ~np.isnan(A)
    a, d, cnt = A[meas], (W @ H)[meas], int(meas.sum())
    if beta == 2:
        t = (a - d) ** 2
        return t.sum() / 2, t.sum() / 2, cnt
    big = a > EPS
    q = a[big] / np.maximum(d[big], EPS)
    if beta == 1:
        t = a[big] * np.log(q)
        return t.sum() - a.sum() + d.sum(), np.abs(t).sum() + a.sum() + d.sum(), cnt
    return q.sum() - cnt - np.log(q).sum(), q.sum() + cnt + np.abs(np.log(q)).sum(), cnt


def fit(A, W0, H0, *, beta, tol=1e-4, max_iter=200, update_W=True, dtype=np.float64):
    """the loop of smk_nmf_masked_dense_device without penalties; returns a dict: W, H, n_iter, converged, error_init, error, margins
    (per check: the stop quantity minus tol, relative to tol)"""
    A = np.asarray(A, dtype=dtype)
    W, H = np.array(W0, dtype=dtype), np.array(H0, dtype=dtype)
    error_of = lambda: np.sqrt(2 * max(divergence(A, W, H, beta)[0], 0))
    error_init = error_of()
    previous, error, checked, margins, converged, it = error_init, error_init, 0, [], False, 0
    for it in range(1, max_iter + 1):
        step_h(A, W, H, beta)
        if update_W:
            step_w(A, W, H, beta)
        if tol > 0 and it % 10 == 0:
            error, checked = error_of(), it
            stop = (previous - error) / error_init
            margins.append(float(abs(stop - tol) / tol))
            if stop < tol:
                converged = True
                break
            previous = error
    if checked != it:
        error = error_of()
    return {"W": np.asarray(W, dtype=np.float64), "H": np.asarray(H, dtype=np.float64), "n_iter": it, "converged": converged,
            "error_init": float(error_init), "error": float(error), "margins": margins}


def step_bar(beta, k, L):
    """tests/beta_reference.step_bar without the power routine's allowance: 4 (c k + L + 8) u, c = max(|beta - 2|, |beta - 1|, 1)"""
    return 4 * (max(abs(beta - 2.0), abs(beta - 1.0), 1.0) * k + L + 8) * U53
