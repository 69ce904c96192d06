#!/usr/bin/env python3
"""A power spectrogram factored on the GPU under the Itakura-Saito divergence (beta = 0), the loss that does not care how loud a
frame is: scikit-learn's NMF(solver="mu", beta_loss="itakura-saito") on a dense matrix that stays in GPU memory, then new frames
folded in against the fitted spectra.

    python examples/is_spectrogram.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import smallk_amd


def synthetic_spectrogram(rng, bins, frames, notes):
    """|STFT|^2 of `notes` harmonic sources that come and go: spectra (bins x notes) with a few decaying partials each, gains
    (notes x frames) that switch on and off and span 40 dB, times exponential (chi-square, 2 degrees of freedom) noise -- the
    multiplicative noise the Itakura-Saito divergence is the likelihood of.  Strictly positive."""
    f = np.arange(bins)[:, None]
    spectra = np.full((bins, notes), 1e-3)
    for j in range(notes):
        f0 = 8 + 5 * j
        for h in range(1, 7):
            spectra[:, j:j + 1] += np.exp(-0.5 * ((f - h * f0) / 1.5) ** 2) / h ** 2
    on = rng.random((notes, frames)) < 0.3
    gains = on * 10.0 ** rng.uniform(-2, 2, (notes, frames)) + 1e-3
    return spectra @ gains * rng.exponential(1.0, (bins, frames)), spectra


def main():
    smallk_amd.initialize(0)
    rng = np.random.default_rng(3)
    bins, frames, new_frames, k = 257, 4000, 500, 8
    V, spectra = synthetic_spectrogram(rng, bins, frames + new_frames, k)
    V_train, V_new = V[:, :frames], V[:, frames:]

    A = smallk_amd.DenseMatrix.from_host(V_train)                      # bins x frames, fp32 storage, both orientations resident
    avg = np.sqrt(V_train.mean() / k)
    W0, H0 = avg * np.abs(rng.standard_normal((bins, k))), avg * np.abs(rng.standard_normal((k, frames)))
    fit = smallk_amd.nmf_beta_dense(A, W0, H0, beta_loss="itakura-saito", tol=1e-4, max_iter=500)
    A.close()
    print(f"{fit.n_iter} iterations, sqrt(2 D_IS(V || W H)) {fit.error_init:.1f} -> {fit.error:.1f}")
    Wn, Sn = fit.W / np.linalg.norm(fit.W, axis=0), spectra / np.linalg.norm(spectra, axis=0)
    print("cosine of each planted spectrum with its best fitted column:", np.round((Sn.T @ Wn).max(axis=1), 3))

    # new frames: only their gains move (update_W=False reads the matrix once per iteration; a single stored copy is enough)
    B = smallk_amd.DenseMatrix.from_host(V_new, single_copy=True)
    Hn0 = np.full((k, new_frames), np.sqrt(V_new.mean() / k))
    new = smallk_amd.nmf_beta_dense(B, fit.W, Hn0, beta_loss=0, update_W=False, tol=1e-4, max_iter=500)
    d = B.beta_divergence(fit.W, new.H, "itakura-saito")
    B.close()
    print(f"{new_frames} new frames folded in over {new.n_iter} iterations: D_IS = {d.divergence:.1f} "
          f"({d.divergence / V_new.size:.3f} per bin; the noise alone costs 0.577 = Euler's constant per bin)")
    # the same numbers as sklearn.decomposition.NMF(solver="mu", beta_loss="itakura-saito", init="custom") on V' from the same
    # start: see tests/test_beta_dense_cpu.py and tests/golden/beta_dense_sklearn.npz


if __name__ == "__main__":
    main()
