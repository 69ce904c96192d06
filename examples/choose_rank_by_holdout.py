#!/usr/bin/env python3
"""Choose the rank of an NMF by hold-out.

The residual on the training matrix falls with every rank added, so it cannot say which rank to use.  The standard answer: withhold a
random share of the entries, fit WITHOUT them, score ON them.  That needs a fit that reads an entry it was not given as "not
measured" -- ``nmf_masked`` -- where every other solver of the library reads it as 0.

A planted rank-5 non-negative matrix with noise, every entry measured; 30 % of the entries are held out.  For k = 2 .. 8 the
held-out error of ``nmf_masked`` has its minimum at the planted rank.  Beside it the score of the fit the library offered before:
``nmf_cd`` on the same training matrix, which takes the withheld entries for zeros and never comes close.

    python examples/choose_rank_by_holdout.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

M, N, RANK, NOISE, HELD_OUT = 300, 200, 5, 0.05, 0.3
KS = range(2, 9)


def make_data(seed=0):
    """(X, the CSC triple of every entry): planted rank + Gaussian noise, clipped at 0 -- a clipped entry is a measured zero"""
    rng = np.random.default_rng(seed)
    W = rng.random((M, RANK)) * (rng.random((M, RANK)) < 0.7)
    H = rng.random((RANK, N)) * (rng.random((RANK, N)) < 0.7)
    X = np.maximum(W @ H + NOISE * rng.standard_normal((M, N)), 0.0)
    indptr = np.arange(N + 1) * M
    indices = np.tile(np.arange(M), N)
    return X, (X.T.reshape(-1).copy(), indices, indptr, (M, N))


def start(k, mean, seed=1):
    rng = np.random.default_rng(seed)
    s = np.sqrt(mean / k)
    return np.abs(rng.standard_normal((M, k))) * s, np.abs(rng.standard_normal((k, N))) * s


def main():
    import smallk_amd
    smallk_amd.initialize(0)
    X, full = make_data()
    train, test = smallk_amd.holdout_split(full, HELD_OUT, seed=3)
    print(f"{M} x {N}, planted rank {RANK}, noise {NOISE}; {train[0].size} entries to fit, {test[0].size} held out "
          f"({(test[0] == 0).sum()} of them measured zeros)")
    A_train, A_test = smallk_amd.SparseMatrix(*train), smallk_amd.SparseMatrix(*test)
    scores = {}
    try:
        print("  k   held-out rmse (nmf_masked)   training rmse   held-out rmse (nmf_cd, zeros for the withheld)")
        for k in KS:
            W0, H0 = start(k, train[0].mean())
            fit = smallk_amd.nmf_masked(A_train, W0, H0, tol=1e-5, max_iter=300)
            held = A_test.masked_residual(fit.W, fit.H)
            seen = A_train.masked_residual(fit.W, fit.H)
            zf = smallk_amd.nmf_cd(A_train, W0, H0, tol=1e-5, max_iter=300)
            held_zf = A_test.masked_residual(zf.W, zf.H)
            scores[k] = held.rmse
            print(f"  {k}   {held.rmse:.5f}                      {seen.rmse:.5f}         {held_zf.rmse:.5f}")
    finally:
        A_train.close()
        A_test.close()
    best = min(scores, key=scores.get)
    print(f"the held-out error is smallest at k = {best} (planted: {RANK}); the training error keeps falling")
    assert best == RANK
    return scores


if __name__ == "__main__":
    main()
