"""The numpy restatement of beta-divergence NMF by multiplicative updates on a dense matrix (include/smallk_amd.h:
smk_nmf_beta_dense_device): scikit-learn 1.7's _fit_multiplicative_update for any beta >= 0 other than 2, in the
library's orientation (A m x n, W m x k, H k x n; W_sklearn = H', components_ = W', sklearn's alpha_W = our alpha_H and the other way
round).  The products are dense matrix products, in any float type (numpy.longdouble), so that the tests can tell what hangs on
rounding.

Per entry a with d = w_i . h_j (EPS = 2^-23):
  qn = a dn^(beta - 2), dn = max(d, EPS) when beta < 2 and d itself above;  qd = dd^(beta - 1), dd = max(d, EPS) when beta < 1
  H step: H[t, j] *= (sum_i W[i, t] qn / den)^gamma, den = sum_i W[i, t] qd (+ l1 if > 0) (+ l2 H[t, j] if > 0), 0 -> EPS
  W step: the same over A' with the new H
  gamma = 1 / (2 - beta) below beta = 1, 1 / (beta - 1) above 2, else 1;  H < 2^-52 -> 0 after its step when beta < 1, W when
  beta <= 1 (sklearn's W and H the other way round)
  beta = 1: qd is not formed, den = the factor's row sums with 0 -> 1 (sklearn's branch; tests/kl_reference.py is its own restatement)
  D over the entries with a > EPS, d clamped at EPS there:  beta = 0: sum a / d - m n - sum log(a / d);  beta = 1: sum a log(a / d)
  - sum a + sum WH;  else (sum a^beta - beta sum a d^(beta - 1) + (beta - 1) sum_all d^beta) / (beta (beta - 1)), the last sum over
  every entry with d as it is.  error = sqrt(2 max(D, 0)), taken before iteration 1 and, when tol > 0, at n_iter = 10, 20, ...:
  stop when (previous_error - error) / error_init < tol.
The powers are written as sklearn writes them (x ** e with a Python float e), so numpy takes the same short cuts: a reciprocal for
-1, a square for 2, a square root for 0.5.
"""
import numpy as np

EPS = 2.0 ** -23            # sklearn's EPSILON: float32's
EPS64 = 2.0 ** -52
U53 = 2.0 ** -53
FIT_BAR = 1e-12             # factors of a whole fit, relative to the largest factor entry (DESIGN 17's bar for cd fits)


def gamma_of(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else 1.0 / (beta - 1.0) if beta > 2 else 1.0


def _update(A, R, X, beta, l1, l2, flush):
    """one half-iteration in place on X (k x cols); A rows x cols, R rows x k the factor of A's rows"""
    beta = float(beta)
    d = R @ X
    dd = None
    if beta != 1:
        dd = d.copy()
        if beta < 1:
            dd[dd < EPS] = EPS
    if beta < 2:
        d[d < EPS] = EPS
    if beta == 1:
        qn = A / d
    elif beta == 0:
        qn = d ** -1.0
        qn = qn ** 2.0
        qn *= A
    else:
        qn = d ** (beta - 2.0)
        qn *= A
    num = R.T @ qn
    if beta == 1:
        s = R.sum(axis=0)
        s[s == 0] = 1.0
        den = np.broadcast_to(s[:, None], X.shape).copy()
    else:
        den = R.T @ (dd ** (beta - 1.0))
    if l1 > 0:
        den += X.dtype.type(l1)
    if l2 > 0:
        den = den + X.dtype.type(l2) * X
    den[den == 0] = EPS
    num /= den
    g = gamma_of(beta)
    if g != 1:
        num **= g
    X *= num
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
    """(D, the sum of the absolute values of the terms D is formed from, the sums themselves as a tuple) -- D not clamped"""
    beta = float(beta)
    A = np.asarray(A, dtype=W.dtype)
    d = W @ H
    keep = A > EPS
    a, dk = A[keep], d[keep]
    dk[dk < EPS] = EPS
    if beta == 0:
        q = a / dk
        lg = np.log(q)
        s1, s2, cnt = q.sum(), lg.sum(), W.dtype.type(A.size)
        return s1 - cnt - s2, abs(s1) + cnt + np.abs(lg).sum(), (s1, s2, cnt)
    if beta == 1:
        t = a * np.log(a / dk)
        s1, swh, sa = t.sum(), d.sum(), a.sum()
        return s1 - sa + swh, np.abs(t).sum() + sa + swh, (s1, swh, sa)
    s1, s2, s3 = (a ** beta).sum(), (a * dk ** (beta - 1.0)).sum(), (d ** beta).sum()
    den = beta * (beta - 1.0)
    return (s1 - beta * s2 + (beta - 1.0) * s3) / den, (s1 + beta * s2 + abs(beta - 1.0) * s3) / abs(den), (s1, s2, s3)


def error_of(A, W, H, beta):
    D = divergence(A, W, H, beta)[0]
    return np.sqrt(2 * max(D, 0))


def fit(A, W0, H0, *, beta, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, tol=1e-3, max_iter=200, update_W=True, dtype=np.float64):
    """the loop of smk_nmf_beta_dense_device; returns a dict: W, H, n_iter, converged, error_init, error, margins (per check: the
    stop quantity minus tol, relative to tol)"""
    dt = np.dtype(dtype)
    A = np.asarray(A, dtype=dt)
    At = np.ascontiguousarray(A.T)
    W = np.array(W0, dtype=dt, order="C")
    H = np.array(H0, dtype=dt, order="C")
    m, n = A.shape
    l1h, l2h = m * alpha_H * l1_ratio, m * alpha_H * (1.0 - l1_ratio)
    l1w, l2w = n * alpha_W * l1_ratio, n * alpha_W * (1.0 - l1_ratio)
    Wt = np.ascontiguousarray(W.T)              # k x m: the W step updates it in place over A'
    error_init = error_of(A, W, H, beta)
    previous, error, checked = error_init, error_init, 0
    margins, converged, it = [], False, 0
    for it in range(1, max_iter + 1):
        _update(A, W, H, beta, l1h, l2h, beta < 1)
        if update_W:
            _update(At, np.ascontiguousarray(H.T), Wt, beta, l1w, l2w, beta <= 1)
            W = np.ascontiguousarray(Wt.T)
        if tol > 0 and it % 10 == 0:
            error, checked = error_of(A, W, H, beta), it
            stop = (previous - error) / error_init
            margins.append(float(abs(stop - tol) / tol))
            if stop < tol:
                converged = True
                break
            previous = error
    if checked != it:
        error = error_of(A, W, H, beta)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return {"W": f64(W), "H": f64(H), "n_iter": it, "converged": converged, "error_init": float(error_init), "error": float(error),
            "margins": margins}


def step_bar(beta, k, L):
    """one step by itself against the longdouble restatement, relative, entry by entry (every summand is non-negative):
    4 (c k + L + 8 + P) u.  c = max(|beta - 2|, |beta - 1|, 1): the rounding of d's k products, amplified by the power; L: the rows
    swept, once per sum; 8: the fixed roundings of the quotients and the update; P = 16 for the power routine of a general beta
    (0 for beta = 0, which takes none) -- a condition on that routine, not a measurement of it."""
    c = max(abs(beta - 2.0), abs(beta - 1.0), 1.0)
    P = 0 if beta == 0 else 16
    return 4 * (c * k + L + 8 + P) * U53
