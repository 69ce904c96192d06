#!/usr/bin/env python3
"""scikit-learn's NMF workflow on the GPU: a document-term matrix in sklearn's orientation (documents x terms), sparse topics
through an L1 penalty, new documents folded in with transform -- coordinate descent, the algorithm sklearn runs by default.

    python examples/sklearn_style_nmf.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import scipy.sparse as sp

import smallk_amd


def main():
    smallk_amd.initialize(0)
    rng = np.random.default_rng(7)
    docs, terms, k = 3000, 2000, 12
    topics = rng.random((k, terms)) * (rng.random((k, terms)) < 0.05)
    weights = rng.random((docs + 200, k)) * (rng.random((docs + 200, k)) < 0.2)
    X = sp.csr_matrix(np.round(4 * weights @ topics))              # term counts
    X_train, X_new = X[:docs], X[docs:]

    for alpha, what in ((0.0, "no penalty"), (2e-3, "alpha_W = alpha_H = 2e-3, l1_ratio = 1")):
        model = smallk_amd.NMF(n_components=k, init="nndsvda", alpha_W=alpha, l1_ratio=1.0, tol=1e-4, max_iter=200)
        W = model.fit_transform(X_train)                            # (documents, k); components_ is (k, terms)
        print(f"{what}: {model.n_iter_} iterations, reconstruction error {model.reconstruction_err_:.2f}, "
              f"{(model.components_ == 0).mean():.0%} of components_ and {(W == 0).mean():.0%} of W exactly zero")
    W_new = model.transform(X_new)                                  # only the new documents' weights move
    dense_new = X_new.toarray()
    print(f"{X_new.shape[0]} new documents folded in: |X_new - W_new components_| / |X_new| = "
          f"{np.linalg.norm(dense_new - model.inverse_transform(W_new)) / np.linalg.norm(dense_new):.3f}")
    # the same numbers as sklearn.decomposition.NMF(solver="cd", init="custom", shuffle=False) from the same start: see
    # tests/test_cd_cpu.py and tests/golden/cd_sklearn.npz


if __name__ == "__main__":
    main()
