"""The cases tests/test_kl_dense_cpu.py and tests/test_gpu_kl_dense.py share: small dense count matrices in
scikit-learn's orientation X (samples x features), the library factors A = X' (features x samples).

Every case (seed s): rng = default_rng(s), lam = Gamma(1, 1)(ns x 4) @ Gamma(1, 1)(4 x nf) scaled to mean 3, X = min(Poisson(lam),
255) -- exact in bf16 and in fp32 --, feature nf - 3 and sample ns - 2 zeroed (a zero row and a zero column of A), the start
avg |N(0, 1)| with avg = sqrt(mean(X) / k), W_sklearn first.  About a fifth of the entries are zeros.  tol = 1e-3, max_iter = 200.
The "real" kind takes lam times Gamma(2, 1/2) noise of mean 1 instead of the Poisson draw, rounded to float32: positive values that are
no integers, for fp32 storage only.  (lam itself has rank 4: a fit of rank 6 meets it almost exactly, D cancels to 1e-4 of its terms
and no summation order holds the error to 1e-12 there.)

The shapes sit on the edges of the kernel's 64 x 64 tile (A is nf x ns, the H step sweeps A, the W step its transpose): one exact
tile (d_k3_l1), one row and one column past a tile (d_k16: 65 x 129), 63 rows (d_tall_k8, d_spans_k8), two 64-row groups of the
factors at k = 65 and 128.
"""
import functools

import numpy as np

TOL, MAX_ITER = 1e-3, 200

# name -> (ns, nf, k, seed, alpha (sklearn's alpha_W, alpha_H = "same"), l1_ratio, kind)
CASES = {
    "d_k2": (70, 130, 2, 21, 0.0, 0.0, "counts"),
    "d_k5": (150, 90, 5, 22, 0.0, 0.0, "counts"),
    "d_k16": (129, 65, 16, 23, 0.0, 0.0, "counts"),
    "d_k17_elastic": (200, 130, 17, 24, 0.01, 0.5, "counts"),
    "d_k33": (200, 130, 33, 25, 0.0, 0.0, "counts"),
    "d_k64": (260, 140, 64, 26, 0.0, 0.0, "counts"),
    "d_k65": (193, 127, 65, 27, 0.0, 0.0, "counts"),
    "d_k128": (260, 140, 128, 28, 0.0, 0.0, "counts"),
    "d_k3_l1": (64, 64, 3, 29, 0.02, 1.0, "counts"),
    "d_tall_k8": (1100, 63, 8, 30, 0.0, 0.0, "counts"),
    # several row tiles per span, the last span short: the launch cuts the row tiles of a column tile into at most 32 spans of
    # equal length (residual_dense_shape).  The W step sweeps A' (2100 x 63): 33 row tiles, one column tile -> 17 spans of 2 tiles,
    # the last of 1.  (The H step sweeps A, 63 x 2100: one row tile.)
    "d_spans_k8": (2100, 63, 8, 31, 0.0, 0.0, "counts"),
    # positive values that are no integers, stored as fp32: the oracle runs on numpy.float32(X)
    "d_real_k6": (100, 70, 6, 32, 0.0, 0.0, "real"),
}
# scikit-learn's n_iter_ on the dense X, recorded when the restatement was checked against it (orders "pair" and "gemm" alike)
SKLEARN_N_ITER = {"d_k2": 40, "d_k5": 80, "d_k16": 120, "d_k17_elastic": 120, "d_k33": 140, "d_k64": 180, "d_k65": 180, "d_k128": 200,
                  "d_k3_l1": 80, "d_tall_k8": 70, "d_spans_k8": 70, "d_real_k6": 60}
GOLDEN_CASES = ("d_k2", "d_k5", "d_k16", "d_k17_elastic", "d_k33", "d_k3_l1")          # k <= 33, within the size limit of a committed file
STEP_CASES = ("d_k16", "d_k64", "d_k65", "d_tall_k8", "d_spans_k8")
SPANS_CASE, REAL_CASE = "d_spans_k8", "d_real_k6"


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: X (ns x nf), A = X' (m x n), W0 (m x k), H0 (k x n), k, kw (the library's keyword arguments), sk (sklearn's), Wsk0 /
    Hsk0 (sklearn's start), storage (what the GPU tests store A as)"""
    ns, nf, k, seed, alpha, l1_ratio, kind = CASES[name]
    rng = np.random.default_rng(seed)
    lam = rng.gamma(1.0, 1.0, (ns, 4)) @ rng.gamma(1.0, 1.0, (4, nf))
    lam *= 3.0 / lam.mean()
    if kind == "real":
        X = (lam * rng.gamma(2.0, 0.5, (ns, nf))).astype(np.float32).astype(np.float64)
    else:
        X = np.minimum(rng.poisson(lam), 255).astype(np.float64)
    X[:, nf - 3] = 0
    X[ns - 2, :] = 0
    avg = np.sqrt(X.mean() / k)
    Wsk = avg * np.abs(rng.standard_normal((ns, k)))
    Hsk = avg * np.abs(rng.standard_normal((k, nf)))
    kw = {"alpha_W": alpha, "alpha_H": alpha, "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER}
    sk = {"alpha_W": alpha, "alpha_H": "same", "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER}
    return {"X": X, "A": np.ascontiguousarray(X.T), "W0": np.ascontiguousarray(Hsk.T), "H0": np.ascontiguousarray(Wsk.T), "k": k, "kw": kw,
            "sk": sk, "Wsk0": Wsk, "Hsk0": Hsk, "storage": "f32"}
