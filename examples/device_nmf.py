#!/usr/bin/env python3
"""Factor a torch tensor that is already in GPU memory and keep the factors there.

A planted low-rank matrix is built on the GPU with torch, handed to the library as it lies (fp32, row-major: no copy to
the host, no fp64 detour), factored with block pivoting, and the factors come back as torch tensors on the same device --
the reconstruction error below is computed by torch without W or H ever visiting the host.

    python examples/device_nmf.py
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
    A = (Ws * (Ws > 0.6)) @ (Hs * (Hs > 0.6)) + 0.01 * torch.rand((m, n), generator=g, device=dev)      # fp32, row-major, in HBM
    W0 = torch.rand((m, k), generator=g, device=dev, dtype=torch.float64)
    H0 = torch.rand((k, n), generator=g, device=dev, dtype=torch.float64)

    # one shot: tensors in, tensors out
    res = smallk_amd.nmf_device(A, W0, H0, "BPP", min_iter=5, max_iter=200, tol=0.005)
    W, H = res.W, res.H
    err = (torch.linalg.norm(A.double() - W @ H) / torch.linalg.norm(A.double())).item()
    print(f"nmf_device: result {res.result}, {res.iteration_count} iterations, W {tuple(W.shape)} on {W.device}, "
          f"H {tuple(H.shape)} on {H.device}, |A - WH| / |A| = {err:.4f}")

    # the same through the objects: the resident matrix serves several solvers, bf16 storage halves its footprint
    D = smallk_amd.DenseMatrix.from_device(A, storage="bf16")
    solver = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n, k, "HALS", min_iter=5, max_iter=50))
    solver.set_factors_device(W0, H0)
    rc, iters, _ = solver.run()
    W, H = solver.factors_device(dtype=torch.float32)
    err = (torch.linalg.norm(A - W @ H) / torch.linalg.norm(A)).item()
    print(f"HALS on bf16 storage: result {rc}, {iters} iterations, fp32 factors on {W.device}, |A - WH| / |A| = {err:.4f}")
    print(f"resident matrix: {D.device_bytes / 2**20:.1f} MiB; stored values back as a tensor: {tuple(D.to_device().shape)}")
    solver.close()
    D.close()


if __name__ == "__main__":
    main()
