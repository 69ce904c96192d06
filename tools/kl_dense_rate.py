#!/usr/bin/env python3
"""What the dense KL-divergence half-iterations and an iteration cost on the device (profiles/kl_dense_rate.txt).

  (a) the fused kernel with its finish alone (smk_kl_dense_step_time): the H step over A, the W step over the stored transpose,
      and the residual pass (launch_residual_dense) on A at the same rank -- ONE product over the same bytes, the floor.  Device
      events around repeated launches, alternating, minimum of three windows.  Reported: the three times, step / residual pass,
      the achieved bytes/s of the one read of A and the fp64 matrix-core FLOP/s of a step.  The expectation is arithmetic: a step
      issues twice the matrix instructions of the residual pass over the same bytes, so a ratio far above 2 at k = 64 would
      mean that the second contraction does not overlap with the loads.
  (b) one whole iteration of nmf_kl_dense, tol = 0.  Host clock around calls that end in a synchronise; per iteration =
      (time of 25 - time of 5) / 20, so set-up cancels.
  (c) orientation only: sklearn.decomposition.NMF(solver="mu", beta_loss="kullback-leibler") on the host at 8192 x 4096, when
      sklearn imports.
Shapes: C3's (65536 x 16384, bf16, k = 32) and 8192 x 4096 at fp32 with k = 16 and k = 64.  Needs a GPU; nothing here falls back
to the CPU.

    python tools/kl_dense_rate.py [--small] [--out profiles/kl_dense_rate.txt]
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


def step_ms(mat, which, k, reps):
    ms = C.c_double(0)
    L.check(L.lib().smk_kl_dense_step_time(mat._h, which, k, reps, C.byref(ms)), "smk_kl_dense_step_time")
    return ms.value


def kernels_alone(mat, m, n, k, ebytes, reps):
    best = {}
    for _ in range(3):
        for which in (2, 0, 1):
            t = step_ms(mat, which, k, reps)
            best[which] = min(best.get(which, t), t)
    kr = 4 if k <= 4 else 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
    tiles = -(-m // 64) * -(-n // 64)
    flops = tiles * 2.0 * (64 * 64 * kr + 64 * 64 * max(kr, 16))          # both contractions as issued, padded rank
    gbytes = m * n * ebytes / 1e9
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of {reps} launches, alternating)")
    say(f"      residual pass over A {best[2]:8.4f} = {gbytes / best[2] * 1e3:7.1f} GB/s of A")
    for which, side in ((0, "H step over A "), (1, "W step over A'")):
        t = best[which]
        say(f"      {side}       {t:8.4f} = {t / best[2]:.2f} x the residual pass, {gbytes / t * 1e3:7.1f} GB/s of the one read, "
            f"{flops / t / 1e9:6.2f} TFLOP/s fp64 MFMA")


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_iteration(run, lo=5, hi=25, n=3):
    run(lo)
    return min((clocked(lambda: run(hi)) - clocked(lambda: run(lo))) / (hi - lo) for _ in range(n))


def iteration(mat, m, n, k):
    g = torch.Generator(device="cuda").manual_seed(2)
    W0 = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64)
    H0 = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float64) * (2.0 / k)
    it = per_iteration(lambda its: smallk_amd.nmf_kl_dense(mat, W0, H0, tol=0.0, max_iter=its))
    say(f"  (b) k = {k}: one iteration of nmf_kl_dense {it * 1e3:.3f} ms from the host clock (two steps, two row sums; no host read between checks)")


def sklearn_case(X, k):
    try:
        from sklearn.decomposition import NMF
    except Exception as e:          # noqa: BLE001
        say(f"  (c) sklearn does not import here ({type(e).__name__}): omitted")
        return
    import warnings
    rng = np.random.default_rng(2)
    W, H = rng.random((X.shape[0], k)) * (2.0 / k), rng.random((k, X.shape[1]))

    def run(it):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            NMF(k, init="custom", solver="mu", beta_loss="kullback-leibler", tol=0.0, max_iter=it).fit_transform(X, W=W.copy(), H=H.copy())
    t1 = time.perf_counter(); run(1); t3 = time.perf_counter(); run(3); t = time.perf_counter()
    say(f"  (c) orientation only: sklearn.decomposition.NMF(solver='mu', beta_loss='kullback-leibler') on the host, same shape, k = {k}: "
        f"{((t - t3) - (t3 - t1)) / 2 * 1e3:.0f} ms per iteration")


def shape(m, n, storage, ks, reps, with_sklearn):
    say(f"dense {m} x {n}, {storage} storage")
    mat = smallk_amd.DenseMatrix(m, n, storage=storage)
    try:
        mat.fill_uniform(7)
        for k in ks:
            kernels_alone(mat, m, n, k, 2 if storage == "bf16" else 4, reps)
            iteration(mat, m, n, k)
        if with_sklearn:
            X = np.ascontiguousarray(mat.download().T)
            sklearn_case(X, ks[0])
    finally:
        mat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the 8192 x 4096 shape only")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.small:
        shape(65536, 16384, "bf16", (32,), 5, False)
    shape(8192, 4096, "f32", (16, 64), 20, not args.no_sklearn)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
