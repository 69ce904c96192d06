"""The numpy restatement of the coordinate-descent sweep and of the NMF loop around it (include/smallk_amd.h: smk_cd_sweep,
smk_nmf_cd_device), and the cases tests/test_cd_cpu.py and tests/test_gpu_cd.py share.

Orientation: A is m x n, W m x k, H k x n.  sklearn.decomposition.NMF(solver="cd", shuffle=False) on X = A' with its alpha_W = our
alpha_H and its alpha_H = our alpha_W is the same iteration, W_sklearn = H' and components_ = W'.

A sweep updates X (k x N, columns independent) for G (k x k), R (k x N), l1, l2: with G' = G + l2 I and R' = R - l1, for
t = 0 .. k-1 in order: grad = G'[t] . x - R'[t]; violation += |x[t] == 0 ? min(0, grad) : grad|; x[t] = max(x[t] - grad / G'[t, t], 0)
unless G'[t, t] == 0.  Two summation orders of the gradient ("seq": r = 0 .. k-1 one after the other, "dot": X' G'[t] as numpy
sums it) and any float type (numpy.longdouble) are available, so that the tests can tell what hangs on rounding.
"""
import numpy as np

U53 = 2.0 ** -53
MARGIN = 2.0 ** -20


class Probe:
    """what the preconditions look at: how far pre-clamp values stay from zero, how far the gradient at a zero entry stays from
    zero, both relative; the smallest over everything seen"""

    def __init__(self):
        self.clamp = np.inf          # min |x - step| / (|x| + |step|)
        self.zero_grad = np.inf      # min over entries with x == 0 of |grad| / (largest |grad| of the column in that sweep)


def sweep(X, G, R, l1, l2, *, order="seq", probe=None):
    """in place on X (k x N, any float dtype); returns the violation"""
    k, N = X.shape
    dt = X.dtype
    Gp = np.array(G, dtype=dt)
    Gp[np.arange(k), np.arange(k)] += dt.type(l2)
    Rp = np.asarray(R, dtype=dt) - dt.type(l1)
    viol = dt.type(0)
    grads = np.zeros((k, N), dtype=dt)
    zeros = np.zeros((k, N), dtype=bool)
    for t in range(k):
        if order == "seq":
            grad = np.zeros(N, dtype=dt)
            for r in range(k):
                grad += Gp[t, r] * X[r]
            grad -= Rp[t]
        else:
            grad = Gp[t] @ X - Rp[t]
        xt = X[t].copy()
        pg = np.where(xt == 0, np.minimum(grad, 0), grad)
        viol += np.abs(pg).sum()
        grads[t], zeros[t] = np.abs(grad), xt == 0
        if Gp[t, t] != 0:
            step = grad / Gp[t, t]
            v = xt - step
            if probe is not None:
                den = np.abs(xt) + np.abs(step)
                live = den > 0
                if live.any():
                    probe.clamp = min(probe.clamp, float(np.min(np.abs(v[live]) / den[live])))
            X[t] = np.maximum(v, 0)
    if probe is not None and zeros.any():
        top = grads.max(axis=0)
        rel = np.where(zeros & (top > 0), grads / np.where(top > 0, top, 1), np.inf)
        probe.zero_grad = min(probe.zero_grad, float(rel.min()))
    return viol


def fit(A, W0, H0, *, alpha_W=0.0, alpha_H=0.0, l1_ratio=0.0, tol=1e-4, max_iter=200, update_W=True, order="seq", dtype=np.float64,
        probe=None):
    """the loop of smk_nmf_cd_device; returns a dict: W, H, n_iter, converged, violation_init, violation, ratios (per iteration)"""
    dt = np.dtype(dtype)
    A = np.asarray(A, dtype=dt)
    m, n = A.shape
    Wt = np.array(np.asarray(W0, dtype=dt).T, order="C")          # k x m, a copy (the transpose of an m x 1 start is contiguous already)
    H = np.array(H0, dtype=dt, order="C")                          # k x n
    l1h, l2h = m * alpha_H * l1_ratio, m * alpha_H * (1.0 - l1_ratio)
    l1w, l2w = n * alpha_W * l1_ratio, n * alpha_W * (1.0 - l1_ratio)
    ratios, v0, v, converged, it = [], None, None, False, 0
    if not update_W:
        Gw, R1 = Wt @ Wt.T, Wt @ A
    for it in range(1, max_iter + 1):
        if update_W:
            Gw, R1 = Wt @ Wt.T, Wt @ A
        v = sweep(H, Gw, R1, l1h, l2h, order=order, probe=probe)
        if update_W:
            v = v + sweep(Wt, H @ H.T, H @ A.T, l1w, l2w, order=order, probe=probe)
        if it == 1:
            v0 = v
        ratios.append(float(v / v0) if v0 != 0 else 0.0)
        if v0 == 0 or v / v0 <= tol:
            converged = True
            break
    return {"W": np.asarray(Wt.T, dtype=np.float64), "H": np.asarray(H, dtype=np.float64), "n_iter": it, "converged": converged,
            "violation_init": float(v0), "violation": float(v), "ratios": ratios}


# ---- the sweep by itself ---------------------------------------------------------------------------------------------------
SWEEP_KS = [1, 3, 16, 17, 32, 33, 64, 65, 128]
SWEEP_NS = [1, 63, 257, 1000]
SWEEP_REGS = ["none", "l1"]


def sweep_case(k, N, reg, seed=1, zero_diag=None):
    """G = F F' / (4 k) for a Gaussian F (k x 4 k): symmetric, well conditioned, off-diagonal entries of both signs.  X: uniform with
    three entries in ten exactly zero; R = G X* + noise for another such X*, so that the gradient at the zeros of X has both
    signs.  reg "l1": l2 = 0.5 and l1 = a quarter of the largest |R|; every fourth column (1, 5, ..) of X and R is scaled by 1 / 64, and those
    columns end as zeros.  zero_diag = t0: row and column t0 of G are zero (use with l2 = 0): x[t0] must stay, its pg counts."""
    rng = np.random.default_rng(7919 * seed + 31 * k + N + (1 if reg == "l1" else 0))
    F = rng.standard_normal((k, 4 * k))
    G = F @ F.T / (4 * k)
    X = rng.random((k, N)) * (rng.random((k, N)) >= 0.3)
    Xs = rng.random((k, N)) * (rng.random((k, N)) >= 0.3)
    R = G @ Xs + 0.1 * rng.standard_normal((k, N))
    l1, l2 = 0.0, 0.0
    if reg == "l1":
        X[:, 1::4] /= 64
        R[:, 1::4] /= 64
        l1, l2 = float(np.abs(R).max()) / 4, 0.5
    if zero_diag is not None:
        G[zero_diag, :] = 0
        G[:, zero_diag] = 0
    return G, R, X, l1, l2


def sweep_bar(k):
    return 64 * k * U53


# ---- fits ------------------------------------------------------------------------------------------------------------------
# name: (m, n, k, alpha_W, alpha_H, l1_ratio, seed, tol); max_iter 200 throughout.  The seeds are the first at which the case holds
# the preconditions of tests/test_cd_cpu.py (a gradient at a zero entry 2^-20 of the column's largest is met once in about a
# million zero entries, and a long run sees that many); tol 1e-3 keeps the sparse case from running on
FIT_MAX_ITER = 200
FIT_CASES = {
    "d96_plain": (96, 70, 5, 0.0, 0.0, 0.0, 1, 1e-4),             # stops after 104 iterations
    "d96_elastic": (96, 70, 5, 1e-3, 2e-3, 0.5, 1, 1e-4),
    "d131_l1": (131, 257, 17, 1e-3, 1e-3, 1.0, 2, 1e-4),          # runs to max_iter
    "d200_mixed": (200, 150, 33, 1e-3, 1e-3, 0.3, 1, 1e-4),       # NNDSVDA start (below): stops after 6
    "s300_sparse": (300, 257, 17, 1e-3, 1e-3, 0.5, 1, 1e-3),      # stops after 119
    "d40_rank1": (40, 30, 1, 0.0, 0.0, 0.0, 1, 1e-4),             # k = 1, and k = 2 on a sparse matrix: the gather product's
    "s65_rank2": (65, 63, 2, 1e-3, 1e-3, 0.5, 1, 1e-4),           # two-row kernel
}
# From a random start the k = 33 case wanders for 150 iterations and the two summation orders of the restatement itself drift
# 7e-14 to 4e-13 of the largest entry apart, past 1 / 16 of the GPU bar at every seed tried: it starts from NNDSVDA instead
# (numpy's SVD, rounded to fp32), where they stay within 2e-14.
NNDSVDA_START = {"d200_mixed"}
GOLDEN_CASES = ["d96_plain", "d96_elastic", "d131_l1"]
RUNS_TO_MAX_ITER = "d131_l1"
FP32_VIEW_CASE = "d96_elastic"
FIT_BAR = 1e-12           # of the largest factor entry
RATIO_BAR = 1e-9


def dense_matrix(m, n, k, seed):
    """planted rank k + integer noise on the grid of 1 / 8: exact in fp32 (entries below 2^8 with three fractional bits)"""
    rng = np.random.default_rng(100 * seed + m + 3 * n + 7 * k)
    Ws = rng.integers(0, 4, (m, k)) * (rng.random((m, k)) < 0.5)
    Hs = rng.integers(0, 4, (k, n)) * (rng.random((k, n)) < 0.5)
    return (Ws @ Hs * 4 + rng.integers(0, 8, (m, n))).astype(np.float64) / 8


def start(m, n, k, mean, seed):
    """W0, H0 > 0 on a grid of 1 / 64 times a power of two near sqrt(mean / k): exact in fp32"""
    rng = np.random.default_rng(500 * seed + m + 3 * n + 7 * k)
    scale = 2.0 ** np.round(np.log2(np.sqrt(mean / k)))
    return rng.integers(1, 128, (m, k)) / 64 * scale, rng.integers(1, 128, (k, n)) / 64 * scale


def fit_case(name):
    """(A dense fp64, csc tuple or None, W0, H0, keyword arguments of fit / nmf_cd's penalties)"""
    m, n, k, aw, ah, rho, seed, tol = FIT_CASES[name]
    csc = None
    if name.startswith("s"):
        import svd_reference
        csc, A = svd_reference.sparse_exact_rank(m, n, k, seed)
    else:
        A = dense_matrix(m, n, k, seed)
    if name in NNDSVDA_START:
        import svd_reference
        U, S, V = svd_reference.numpy_svd(A, k)
        W0, H0 = svd_reference.nndsvd_from_svd(U, S[:k], V, variant="nndsvda", mean=A.mean())
        W0, H0 = W0.astype(np.float32).astype(np.float64), H0.astype(np.float32).astype(np.float64)
    else:
        W0, H0 = start(m, n, k, A.mean(), seed)
    return A, csc, W0, H0, {"alpha_W": aw, "alpha_H": ah, "l1_ratio": rho, "tol": tol, "max_iter": FIT_MAX_ITER}
