#!/usr/bin/env python3
"""What the KL-divergence half-iterations and a KL iteration cost on the device (profiles/kl_rate.txt).

  (a) the quotient-gather kernel alone (with its update epilogue and fix-up) against launch_spmm_seg on the same plan, rank and
      gathered factor (smk_kl_step_time): the plain gather is one read of the same rows without the dot product and the quotient,
      so the ratio is what fusing them costs over that floor.  Both sides (CSC(A) for H, CSC(A') for W), device events around
      repeated launches, alternating, minimum of three windows.
  (b) one iteration: nmf_kl against nmf_cd on the same matrix, tol = 0.  Host clock around calls that end in a synchronise; per
      iteration = (time of 25 - time of 5) / 20, so set-up cancels.
  (c) orientation only: sklearn.decomposition.NMF(solver="mu", beta_loss="kullback-leibler") on the host, when sklearn imports.
Shapes: the s_reuters shape (sparse 12411 x 7984) and the 10^6-column community graph of s_1m, k = 32.  Needs a GPU; nothing here
falls back to the CPU.

    python tools/kl_rate.py [--small] [--out profiles/kl_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd
from smallk_amd import _lib as L

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def step_ms(mat, which, k, reps=20):
    ms = C.c_double(0)
    L.check(L.lib().smk_kl_step_time(mat._h, which, k, reps, C.byref(ms)), "smk_kl_step_time")
    return ms.value


def kernels_alone(mat, k):
    best = {}
    for _ in range(3):
        for which in (2, 0, 3, 1):
            t = step_ms(mat, which, k)
            best[which] = min(best.get(which, t), t)
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of 20 launches, alternating)")
    say(f"      H side, CSC(A):  plain gather {best[2]:8.4f} | quotient gather + update {best[0]:8.4f} = {best[0] / best[2]:.2f} x the gather")
    say(f"      W side, CSC(A'): plain gather {best[3]:8.4f} | quotient gather + update {best[1]:8.4f} = {best[1] / best[3]:.2f} x the gather")


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_iteration(run, lo=5, hi=25, n=3):
    run(lo)
    return min((clocked(lambda: run(hi)) - clocked(lambda: run(lo))) / (hi - lo) for _ in range(n))


def iterations(mat, m, n, k):
    g = torch.Generator(device="cuda").manual_seed(2)
    W0 = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64)
    H0 = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float64) * (2.0 / k)
    kl = per_iteration(lambda it: smallk_amd.nmf_kl(mat, W0, H0, tol=0.0, max_iter=it))
    cd = per_iteration(lambda it: smallk_amd.nmf_cd(mat, W0, H0, tol=0.0, max_iter=it))
    say(f"  (b) k = {k}: one KL iteration {kl * 1e3:.3f} ms (no host read between checks) | one cd iteration {cd * 1e3:.3f} ms (the violation read "
        f"every iteration) | KL / cd = {kl / cd:.2f}")


def sklearn_case(A, k):
    try:
        from sklearn.decomposition import NMF
    except Exception as e:          # noqa: BLE001
        say(f"  (c) sklearn does not import here ({type(e).__name__}): omitted")
        return
    import warnings
    X = A.T.tocsr()
    rng = np.random.default_rng(2)
    W, H = rng.random((X.shape[0], k)) * (2.0 / k), rng.random((k, X.shape[1]))

    def run(it):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            NMF(k, init="custom", solver="mu", beta_loss="kullback-leibler", tol=0.0, max_iter=it).fit_transform(X, W=W.copy(), H=H.copy())
    t2 = time.perf_counter(); run(2); t6 = time.perf_counter(); run(6); t = time.perf_counter()
    say(f"  (c) orientation only: sklearn.decomposition.NMF(solver='mu', beta_loss='kullback-leibler') on the host, same shape: "
        f"{((t - t6) - (t6 - t2)) / 4 * 1e3:.1f} ms per iteration")


def shape(name, k, with_sklearn):
    import bench_sparse
    A = bench_sparse.make_matrix(name).tocsc()
    A.sum_duplicates()
    A.data = np.abs(A.data)
    m, n = A.shape
    say(f"{name}: sparse {m} x {n}, {A.nnz} stored entries")
    S = smallk_amd.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    try:
        kernels_alone(S, k)
        iterations(S, m, n, k)
    finally:
        S.close()
    if with_sklearn:
        sklearn_case(A, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the s_reuters shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    shape("s_reuters", 32, True)
    if not args.small:
        shape("s_1m", 32, False)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
