#!/usr/bin/env python3
"""Start a factorisation from NNDSVD instead of random numbers: a tensor in GPU memory in, the deterministic SVD-based start
built on the device, block pivoting from it, and the reconstruction error before and after -- nothing visits the host.

    python examples/nndsvd_init.py
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
    m, n, k = 4096, 2048, 16
    Ws = torch.rand((m, k), generator=g, device=dev)
    Hs = torch.rand((k, n), generator=g, device=dev)
    A = (Ws * (Ws > 0.6)) @ (Hs * (Hs > 0.6)) + 0.01 * torch.rand((m, n), generator=g, device=dev)

    D = smallk_amd.DenseMatrix.from_device(A)
    U, S, V = D.svd(k)                                   # the spectrum a user would pick k from
    print("leading singular values:", " ".join(f"{s:.1f}" for s in S[:6]), "...")
    W0, H0 = D.nndsvd(k)                                 # float64 tensors on the GPU, the same on every run
    print(f"NNDSVD start:   |A - W0 H0| / |A| = {D.residual(W0, H0).relative:.4f}")

    solver = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n, k, "BPP"))
    solver.set_factors_nndsvd()                          # the same start, handed over on the device
    solver.iterate(10)
    print(f"10 BPP iterations: |A - W H| / |A| = {solver.residual().relative:.4f}")
    solver.set_factors_uniform(1, 2)
    solver.iterate(10)
    print(f"  (from uniform random factors:      {solver.residual().relative:.4f})")
    solver.close()
    D.close()


if __name__ == "__main__":
    main()
