"""The cases tests/test_kl_cpu.py and tests/test_gpu_kl.py share: small term-document count matrices in
scikit-learn's orientation X (samples x features), the library factors A = X' (features x samples).

Every case: p = min(1, P / (f + 1)) per feature f, M = (uniform < p) * integers in 1 .. 5, feature nf - 3 and sample ns - 2
emptied (an empty row and an empty column of A), the start avg |N(0, 1)| with avg = sqrt(mean(X) / k), W_sklearn first.  With
P = 40 every column of A (a sample) holds more entries than one segment of 64 and so does every frequent row: both sweeps have
long-column pieces.  With P = 8 no column of A exceeds a segment.  tol = 1e-3, max_iter = 200 throughout.
"""
import functools

import numpy as np

TOL, MAX_ITER = 1e-3, 200
SEG = 64                  # entries per segment of the library's plans (the default of SMK_SPMM_SEG_LEN)

# name -> (ns, nf, k, seed, alpha (sklearn's alpha_W, alpha_H = "same"), l1_ratio, P, kind)
CASES = {
    "k5": (150, 90, 5, 1, 0.0, 0.0, 40, "plain"),
    "k16": (150, 90, 16, 2, 0.0, 0.0, 40, "plain"),
    "k17_elastic": (200, 130, 17, 3, 0.01, 0.5, 40, "plain"),
    "k33": (200, 130, 33, 4, 0.0, 0.0, 40, "plain"),
    "k64": (260, 140, 64, 5, 0.0, 0.0, 40, "plain"),
    "k3_l1": (150, 90, 3, 6, 0.02, 1.0, 40, "plain"),
    "k128": (260, 140, 128, 7, 0.0, 0.0, 40, "plain"),
    "k2": (150, 90, 2, 8, 0.0, 0.0, 40, "plain"),
    # no column of A longer than a segment: no pieces on the H side
    "short_k8": (150, 200, 8, 9, 0.0, 0.0, 8, "plain"),
    # component 1 of W0 all zero, H0 zero on the non-empty column 3: the clamps, the 0 -> 1.0 and the 0 -> EPS rule
    "degenerate_k4": (150, 90, 4, 10, 0.0, 0.0, 40, "degenerate"),
    # k = min(m, n)
    "kmin_k30": (60, 30, 30, 11, 0.0, 0.0, 40, "plain"),
}
# scikit-learn's n_iter_ on the cases of the issue, recorded when the restatement was checked against it
SKLEARN_N_ITER = {"k5": 90, "k16": 160, "k17_elastic": 110, "k33": 140, "k64": 200, "k3_l1": 70, "k128": 200, "k2": 50}
GOLDEN_CASES = ("k5", "k16", "k17_elastic", "k33", "k3_l1", "k2")
TRANSFORM_CASE = "k5"            # the golden holds sklearn's transform of this case's own X
DEGENERATE_COMPONENT, DEGENERATE_COLUMN = 1, 3


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: X (ns x nf), A = X' (m x n), csc = (vals, rows, indptr, (m, n)) of A, W0 (m x k), H0 (k x n), k, kw (the library's
    keyword arguments), sk (sklearn's)"""
    ns, nf, k, seed, alpha, l1_ratio, P, kind = CASES[name]
    rng = np.random.default_rng(seed)
    p = np.minimum(1.0, P / (np.arange(nf) + 1.0))
    M = (rng.random((ns, nf)) < p) * rng.integers(1, 6, (ns, nf))
    M[:, nf - 3] = 0
    M[ns - 2, :] = 0
    X = M.astype(np.float64)
    avg = np.sqrt(X.mean() / k)
    Wsk = avg * np.abs(rng.standard_normal((ns, k)))
    Hsk = avg * np.abs(rng.standard_normal((k, nf)))
    if kind == "degenerate":
        Hsk[DEGENERATE_COMPONENT, :] = 0.0           # W0[:, 1] = 0
        assert X[DEGENERATE_COLUMN].sum() > 0
        Wsk[DEGENERATE_COLUMN, :] = 0.0              # H0[:, 3] = 0
    A = np.ascontiguousarray(X.T)
    # the CSC of A is the CSR of X: sample by sample, features ascending
    indptr = np.concatenate([[0], np.cumsum((X != 0).sum(axis=1))]).astype(np.int64)
    sj, fi = np.nonzero(X)
    csc = (X[sj, fi].copy(), fi.astype(np.int64), indptr, (nf, ns))
    kw = {"alpha_W": alpha, "alpha_H": alpha, "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER}
    sk = {"alpha_W": alpha, "alpha_H": "same", "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER}
    return {"X": X, "A": A, "csc": csc, "W0": np.ascontiguousarray(Hsk.T), "H0": np.ascontiguousarray(Wsk.T), "k": k, "kw": kw, "sk": sk,
            "Wsk0": Wsk, "Hsk0": Hsk}


def longest(A):
    """(longest column, longest row) of A in stored entries"""
    nz = A != 0
    return int(nz.sum(axis=0).max()), int(nz.sum(axis=1).max())
