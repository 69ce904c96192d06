#!/usr/bin/env python3
"""Topics of count data on the GPU under the loss made for counts: scikit-learn's NMF(solver="mu", beta_loss="kullback-leibler")
workflow -- PLSA's objective -- on a sparse document-term matrix in sklearn's orientation (documents x terms), new documents
folded in with transform.

    python examples/kl_topics.py
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
    X = sp.csr_matrix(rng.poisson(4 * weights @ topics).astype(np.float64))       # term counts
    X_train, X_new = X[:docs], X[docs:]

    model = smallk_amd.NMF(n_components=k, solver="mu", beta_loss="kullback-leibler", init="nndsvda", tol=1e-4, max_iter=200)
    W = model.fit_transform(X_train)                                # (documents, k); components_ is (k, terms)
    print(f"{model.n_iter_} iterations, sqrt(2 D(X || W H)) = {model.reconstruction_err_:.2f}, "
          f"{(model.components_ == 0).mean():.0%} of components_ exactly zero")
    top = np.argsort(-model.components_, axis=1)[:, :5]
    truth = np.argsort(-topics, axis=1)[:, :50]
    found = [max(len(set(t) & set(u)) for u in truth) for t in top]
    print(f"top 5 terms of each fitted topic that are among the top 50 of one planted topic: {found}")
    W_new = model.transform(X_new)                                  # only the new documents' weights move
    mat = smallk_amd.SparseMatrix.from_scipy(X_new.T.tocsc())
    d = mat.kl_divergence(model.components_.T, W_new.T)
    mat.close()
    print(f"{X_new.shape[0]} new documents folded in: D(X_new || W_new components_) = {d.divergence:.1f} over {X_new.nnz} stored counts")
    # the same numbers as sklearn.decomposition.NMF(solver="mu", beta_loss="kullback-leibler", init="custom") from the same start:
    # see tests/test_kl_cpu.py and tests/golden/kl_sklearn.npz


if __name__ == "__main__":
    main()
