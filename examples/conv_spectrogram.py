#!/usr/bin/env python3
"""Convolutive NMF on the device (smallk_amd.nmf_conv_dense): two patterns of T = 6 columns -- a rising and a falling
chirp -- are planted at random onsets in a 48 x 400 "spectrogram" and recovered from a random start; plain NMF at the same k = 2 has
one column per component and cannot describe either.  Needs a GPU.

    python examples/conv_spectrogram.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd

m, n, k, T = 48, 400, 2, 6
rng = np.random.default_rng(3)
P = np.zeros((T, m, k))
for t in range(T):
    P[t, 8 + 3 * t:12 + 3 * t, 0] = 1.0 - 0.1 * t           # the rising chirp
    P[t, 40 - 4 * t:43 - 4 * t, 1] = 0.5 + 0.1 * t           # the falling one
onsets = np.zeros((k, n))
for r in range(k):
    onsets[r, rng.choice(n - T, 12, replace=False)] = rng.uniform(0.5, 2.0, 12)
A = 0.01 + sum(P[t] @ np.pad(onsets, ((0, 0), (t, 0)))[:, :n] for t in range(T))

smallk_amd.initialize(0)
mat = smallk_amd.DenseMatrix.from_host(A)
start = lambda *shape: torch.from_numpy(rng.uniform(0.1, 1.0, shape)).cuda()
conv = smallk_amd.nmf_conv_dense(mat, start(T, m, k), start(k, n), beta_loss="kullback-leibler", tol=0.0, max_iter=300)
plain = smallk_amd.nmf_kl_dense(mat, start(m, k), start(k, n), tol=0.0, max_iter=300)
mat.close()

W = conv.W.cpu().numpy()
cosine = lambda a, b: float(a.ravel() @ b.ravel() / np.linalg.norm(a) / np.linalg.norm(b))
print(f"sqrt(2 D_KL): convolutive k = {k}, T = {T}: {conv.error:.2f}    plain NMF k = {k}: {plain.error:.2f}    (start {conv.error_init:.1f})")
for r, name in enumerate(("rising chirp", "falling chirp")):
    print(f"{name}: cosine with the closest fitted pattern {max(cosine(P[:, :, r], W[:, :, q]) for q in range(k)):.4f}")
