#!/usr/bin/env python3
"""Raw term counts in, labels out: fit the term set and idf on one batch of documents, train topics on the fit's matrix, and
label a later batch of raw counts with them.  After its upload the new batch never returns to the host.

``preprocess`` prunes the training counts and scores them (tf-idf); ``result.vocabulary()`` keeps what the fit learnt -- the
surviving terms, their idf -- on the device; ``Vocabulary.apply`` turns the later batch, still in the original term numbering,
into the matrix of the trained term space; ``transform`` folds it into the trained W and ``labels_device`` labels it.

    python examples/classify_raw_documents.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import smallk_amd
from smallk_amd.preprocess import preprocess
from smallk_amd.synthetic import term_counts


def main():
    smallk_amd.initialize(0)
    m, n, k = 5000, 3000, 8
    A = term_counts(m, n, 20 * n, 3, dup_frac=0.05).tocsc()
    n_train = 2 * n // 3
    train, new = A[:, :n_train], A[:, n_train:]

    # fit: pruning and tf-idf of the training counts; the reduced matrix stays on the device
    fit = preprocess(m, n_train, train.indptr, train.indices, train.data)
    print(f"fit: {m} terms x {n_train} documents -> {fit.height} x {fit.width} after {fit.iterations} iterations")
    A_fit = fit.matrix()
    solver = smallk_amd.NmfSolver(A_fit, smallk_amd.make_options(fit.height, fit.width, k, "BPP", min_iter=5, max_iter=50))
    solver.set_factors_uniform(1, 2)
    rc, iters, _ = solver.run()
    W, _ = solver.factors_device(normalize=True)
    sizes = torch.bincount(solver.labels_device().long(), minlength=k).tolist()
    print(f"trained: result {rc}, {iters} iterations; cluster sizes {sizes}")

    # later documents: raw counts in the original term numbering -> the fit's term space, the fit's idf
    vocab = fit.vocabulary()
    applied = vocab.apply(new, min_terms=1)
    print(f"new documents: {new.shape[1]} raw, {applied.width} with a known term, {applied.nnz} of {new.nnz} entries in the "
          f"vocabulary; upload {applied.upload_ms:.2f} ms, device {applied.device_ms:.2f} ms")
    A_new = applied.matrix()
    H_new = smallk_amd.transform(A_new, W)
    labels = smallk_amd.labels_device(H_new)
    print(f"labelled on {labels.device}: cluster sizes {torch.bincount(labels.long(), minlength=k).tolist()}, "
          f"|A_new - W H_new| / |A_new| = {A_new.residual(W, H_new).relative:.4f}")
    solver.close()
    for x in (A_new, A_fit, applied, vocab, fit):
        x.close()


if __name__ == "__main__":
    main()
