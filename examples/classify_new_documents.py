#!/usr/bin/env python3
"""Train topics on one term-document matrix, label a second batch of documents with them -- everything stays on the GPU.

A planted matrix is split by columns into a training set and a batch of new documents.  The training set is factored with
block pivoting; ``transform`` folds the new documents into the trained W (H_new = argmin_{H >= 0} ||A_new - W H||_F, one exact
solve); ``labels_device`` and ``top_terms_device`` turn the factors into cluster labels, memberships and the topics' top terms
as torch tensors.  Nothing but the few numbers printed below crosses to the host.

    python examples/classify_new_documents.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import smallk_amd


def main():
    smallk_amd.initialize(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    m, n_train, n_new, k = 4096, 2048, 300, 16
    Ws = torch.rand((m, k), generator=g, device=dev)
    Hs = torch.rand((k, n_train + n_new), generator=g, device=dev)
    A = (Ws * (Ws > 0.7)) @ (Hs * (Hs > 0.7)) + 0.01 * torch.rand((m, n_train + n_new), generator=g, device=dev)
    A_train, A_new = A[:, :n_train], A[:, n_train:]              # column slices of a row-major tensor: taken as they lie

    # train
    D = smallk_amd.DenseMatrix.from_device(A_train)
    solver = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n_train, k, "BPP", min_iter=5, max_iter=100))
    solver.set_factors_device(torch.rand((m, k), generator=g, device=dev, dtype=torch.float64),
                              torch.rand((k, n_train), generator=g, device=dev, dtype=torch.float64))
    rc, iters, _ = solver.run()
    W, _ = solver.factors_device(normalize=True)
    labels = solver.labels_device()                               # of the resident H, no copy of it
    terms = solver.top_terms_device(5)
    print(f"trained: result {rc}, {iters} iterations; cluster sizes {torch.bincount(labels.long(), minlength=k).tolist()}")
    for j in range(3):
        print(f"  topic {j}: top terms {terms[j].tolist()}")

    # classify the new documents with the trained W
    N = smallk_amd.DenseMatrix.from_device(A_new)
    H_new = smallk_amd.transform(N, W)
    new_labels, P = smallk_amd.labels_device(H_new, memberships=True)
    planted = Hs[:, n_train:].argmax(0)
    same = torch.zeros((k, k), device=dev)
    same.index_put_((new_labels.long(), planted), torch.ones(n_new, device=dev), accumulate=True)
    print(f"new documents: {n_new} labelled on {new_labels.device}, |A_new - W H_new| / |A_new| = {N.residual(W, H_new).relative:.4f}")
    print(f"  documents whose label is their cluster's most frequent planted topic: {int(same.max(1).values.sum())} of {n_new}")
    print(f"  memberships of document 0: {[round(x, 3) for x in P[:, 0].tolist()]}")
    solver.close()
    N.close()
    D.close()


if __name__ == "__main__":
    main()
