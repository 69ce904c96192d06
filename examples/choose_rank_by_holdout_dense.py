#!/usr/bin/env python3
"""Choose the rank of an Itakura-Saito NMF of a dense matrix by hold-out.

``choose_rank_by_holdout.py`` for the losses a spectrogram is fitted under: the divergence on the training matrix falls with every
rank added, so a random share of the entries is withheld, the fit is made WITHOUT them and scored ON them.  On a dense matrix "not
measured" is a stored NaN: ``holdout_split_dense`` returns two arrays with complementary NaNs, ``nmf_masked_dense`` fits the
measured entries of the first and ``DenseMatrix.masked_divergence`` scores the measured entries of the second.

A planted rank-4 strictly positive matrix with multiplicative Gamma noise (what the Itakura-Saito loss models), 5 % of the entries
unmeasured from the start, 30 % of the rest held out.  For k = 2 .. 7 the mean held-out divergence has its minimum at the planted
rank while the training divergence keeps falling.

    python examples/choose_rank_by_holdout_dense.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

M, N, RANK, SHAPE, HELD_OUT = 300, 200, 4, 10.0, 0.3
KS = range(2, 8)


def make_data(seed=0):
    """planted rank times Gamma(SHAPE, 1 / SHAPE) noise of mean 1, then 5 % dead entries"""
    rng = np.random.default_rng(seed)
    X = (0.05 + rng.random((M, RANK))) @ (0.05 + rng.random((RANK, N))) * rng.gamma(SHAPE, 1.0 / SHAPE, (M, N))
    X[rng.random((M, N)) < 0.05] = np.nan
    return X


def start(k, mean, seed=1):
    rng = np.random.default_rng(seed)
    s = np.sqrt(mean / k)
    return np.abs(rng.standard_normal((M, k))) * s, np.abs(rng.standard_normal((k, N))) * s


def main():
    import smallk_amd
    smallk_amd.initialize(0)
    X = make_data()
    train, test = smallk_amd.holdout_split_dense(X, HELD_OUT, seed=3)
    print(f"{M} x {N}, planted rank {RANK}; {int((~np.isnan(train)).sum())} entries to fit, {int((~np.isnan(test)).sum())} held out, "
          f"{int(np.isnan(X).sum())} never measured")
    A_train, A_test = smallk_amd.DenseMatrix.from_host(train), smallk_amd.DenseMatrix.from_host(test)
    scores = {}
    try:
        print("  k   mean held-out divergence   mean training divergence")
        for k in KS:
            W0, H0 = start(k, np.nanmean(train))
            fit = smallk_amd.nmf_masked_dense(A_train, W0, H0, beta_loss="itakura-saito", tol=1e-5, max_iter=500, precision="fp32")
            held = A_test.masked_divergence(fit.W, fit.H, "itakura-saito")
            seen = A_train.masked_divergence(fit.W, fit.H, "itakura-saito")
            scores[k] = held.mean
            print(f"  {k}   {held.mean:.5f}                    {seen.mean:.5f}")
    finally:
        A_train.close()
        A_test.close()
    best = min(scores, key=scores.get)
    print(f"the held-out divergence is smallest at k = {best} (planted: {RANK}); the training divergence keeps falling")
    assert best == RANK
    return scores


if __name__ == "__main__":
    main()
