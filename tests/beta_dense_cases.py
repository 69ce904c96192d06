"""The cases tests/test_beta_dense_cpu.py and tests/test_gpu_beta_dense.py share: small dense matrices in
scikit-learn's orientation X (samples x features), the library factors A = X' (features x samples).  The generator is
tests/kl_dense_cases.py's: rng = default_rng(seed), lam = Gamma(1, 1)(ns x 4) @ Gamma(1, 1)(4 x nf) scaled to mean 3, the start
avg |N(0, 1)| with avg = sqrt(mean(X) / k), W_sklearn first; tol = 1e-3, max_iter = 200.

"real":   X = lam times Gamma(2, 1/2) noise of mean 1, rounded to float32, with NO zeroed row or column: strictly positive, what
          beta = 0 (Itakura-Saito) needs.  fp32 storage.
"counts": X = min(Poisson(lam), 255) with feature nf - 3 and sample ns - 2 zeroed (a zero row and a zero column of A), for the
          betas that take zeros.

The shapes sit on the edges of the kernel's 64 x 64 tile as in kl_dense_cases: one exact tile (is_k3_tile), one row and one column
past a tile (is_k16: A is 65 x 129), 63 rows (is_tall_k8, is_spans_k8: the W step sweeps 33 row tiles in 17 spans), two 64-row
groups of the factors at k = 65 and 128.
"""
import functools

import numpy as np

TOL, MAX_ITER = 1e-3, 200

# name -> (ns, nf, k, seed, beta, alpha (sklearn's alpha_W, alpha_H = "same"), l1_ratio, kind)
CASES = {
    "is_k2": (70, 130, 2, 41, 0.0, 0.0, 0.0, "real"),
    "is_k5": (150, 90, 5, 42, 0.0, 0.0, 0.0, "real"),
    "is_k16": (129, 65, 16, 57, 0.0, 0.0, 0.0, "real"),
    "is_k33": (200, 130, 33, 44, 0.0, 0.0, 0.0, "real"),
    "is_k64": (260, 140, 64, 45, 0.0, 0.0, 0.0, "real"),
    "is_k65": (193, 127, 65, 46, 0.0, 0.0, 0.0, "real"),
    "is_k128": (260, 140, 128, 47, 0.0, 0.0, 0.0, "real"),
    "is_tall_k8": (1100, 63, 8, 48, 0.0, 0.0, 0.0, "real"),
    "is_spans_k8": (2100, 63, 8, 49, 0.0, 0.0, 0.0, "real"),
    "is_k3_tile": (64, 64, 3, 50, 0.0, 0.0, 0.0, "real"),
    "b05_k17": (200, 130, 17, 51, 0.5, 0.0, 0.0, "counts"),
    "b15_k33": (200, 130, 33, 52, 1.5, 0.0, 0.0, "counts"),
    "b3_k9": (129, 65, 9, 53, 3.0, 0.0, 0.0, "counts"),
    "b05_k65": (193, 127, 65, 54, 0.5, 0.0, 0.0, "real"),
    "b15_k16_el": (129, 65, 16, 55, 1.5, 0.01, 0.5, "counts"),
}
# scikit-learn 1.7.2's n_iter_ on X, recorded when the restatement was checked against it
SKLEARN_N_ITER = {"is_k2": 60, "is_k5": 110, "is_k16": 180, "is_k33": 200, "is_k64": 200, "is_k65": 200, "is_k128": 200, "is_tall_k8": 110,
                  "is_spans_k8": 100, "is_k3_tile": 80, "b05_k17": 150, "b15_k33": 160, "b3_k9": 160, "b05_k65": 200, "b15_k16_el": 140}
# the recorded sklearn results: cases with k <= 33 whose factors together stay below the size of tests/golden/kl_sklearn.npz (random
# float64 does not compress) -- every beta of the table and the elastic-net case; is_k33, b15_k33 and the two tall cases are left to
# live sklearn
GOLDEN_CASES = ("is_k2", "is_k5", "is_k16", "is_k3_tile", "b05_k17", "b3_k9", "b15_k16_el")
STEP_CASES = ("is_k16", "is_k64", "is_k65", "is_tall_k8", "is_spans_k8", "b05_k17", "b3_k9")
DIVERGENCE_CASES = ("is_k5", "is_k65", "is_spans_k8", "b05_k17", "b3_k9")
SPANS_CASE, BF16_CASE = "is_spans_k8", "is_k5"


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: X (ns x nf), A = X' (m x n), W0 (m x k), H0 (k x n), k, beta, kw (the library's keyword arguments, beta_loss among
    them), ref (tests/beta_reference.fit's), sk (sklearn's), Wsk0 / Hsk0 (sklearn's start), storage (what the GPU tests store A as)"""
    ns, nf, k, seed, beta, alpha, l1_ratio, kind = CASES[name]
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
    pen = {"alpha_W": alpha, "alpha_H": alpha, "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER}
    sk = {"alpha_W": alpha, "alpha_H": "same", "l1_ratio": l1_ratio, "tol": TOL, "max_iter": MAX_ITER, "beta_loss": beta}
    return {"X": X, "A": np.ascontiguousarray(X.T), "W0": np.ascontiguousarray(Hsk.T), "H0": np.ascontiguousarray(Wsk.T), "k": k, "beta": beta,
            "kw": dict(pen, beta_loss=beta), "ref": dict(pen, beta=beta), "sk": sk, "Wsk0": Wsk, "Hsk0": Hsk, "storage": "f32"}
