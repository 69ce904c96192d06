"""Convolutive NMF (smallk_amd.nmf_conv_dense) restated in plain numpy with explicit shifted dense products, in
whatever float type the factors have (float64 or longdouble): the model sum_t W[t] shift_t(H), the H step, the W step with the new H,
the divergence and the iteration with its stopping rule.  W is (T, m, k), H is (k, n), beta is 0 (Itakura-Saito) or 1 (KL)."""
import numpy as np

EPS = 2.0 ** -23          # scikit-learn's EPSILON: the clamp of the model
EPS64 = 2.0 ** -52        # below it an updated entry becomes zero
U53 = 2.0 ** -53


def shift(X, t):
    """columns moved t places to the right (t < 0: to the left), zeros entering"""
    S = np.zeros_like(X)
    n = X.shape[1]
    if t >= 0:
        S[:, t:] = X[:, :n - t]
    else:
        S[:, :n + t] = X[:, -t:]
    return S


def model(W, H):
    return sum(W[t] @ shift(H, t) for t in range(W.shape[0]))


def _quotients(A, W, H, beta):
    d = np.maximum(model(W, H), EPS)
    return (A / d, np.ones_like(d)) if beta == 1 else (A / (d * d), 1 / d)


def _update(x, num, den, l1, l2, beta, flush):
    den = den + l1 + l2 * x
    q = num / np.where(den == 0, EPS, den)
    xn = x * (q if beta == 1 else np.sqrt(q))
    return np.where(xn < EPS64, 0, xn) if flush else xn


def step_h(A, W, H, beta, l1=0.0, l2=0.0):
    qn, qd = _quotients(A, W, H, beta)
    num = sum(shift(W[t].T @ qn, -t) for t in range(W.shape[0]))
    den = sum(shift(W[t].T @ qd, -t) for t in range(W.shape[0]))
    return _update(H, num, den, l1, l2, beta, beta == 0)


def step_w(A, W, H, beta, l1=0.0, l2=0.0):
    qn, qd = _quotients(A, W, H, beta)
    return np.stack([_update(W[t], qn @ shift(H, t).T, qd @ shift(H, t).T, l1, l2, beta, True) for t in range(W.shape[0])])


def divergence(A, W, H, beta):
    """(D, the sum of the absolute values of the terms D is formed from) over the entries with a > EPS"""
    lam = model(W, H)
    live = A > EPS
    a, d = A[live], np.maximum(lam, EPS)[live]
    if beta == 1:
        terms = [a * np.log(a / d), -a, lam]
    else:
        terms = [a / d, -np.log(a / d), -np.ones_like(A)]
    return sum(t.sum() for t in terms), sum(np.abs(t).sum() for t in terms)


def fit(A, W, H, beta, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True):
    m, n = A.shape
    l1h, l2h, l1w, l2w = m * alpha_H * l1_ratio, m * alpha_H * (1 - l1_ratio), n * alpha_W * l1_ratio, n * alpha_W * (1 - l1_ratio)
    err = lambda: np.sqrt(2 * max(divergence(A, W, H, beta)[0], 0))
    e0 = prev = e = err()
    it, conv, checked = 0, False, 0
    for it in range(1, max_iter + 1):
        H = step_h(A, W, H, beta, l1h, l2h)
        if update_W:
            W = step_w(A, W, H, beta, l1w, l2w)
        if tol > 0 and it % 10 == 0:
            e, checked = err(), it
            if (prev - e) / e0 < tol:
                conv = True
                break
            prev = e
    if checked != it:
        e = err()
    return dict(W=W, H=H, n_iter=it, converged=conv, error_init=float(e0), error=float(e))
