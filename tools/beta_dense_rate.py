#!/usr/bin/env python3
"""What the dense beta-divergence half-iterations and an iteration cost on the device (profiles/beta_dense_rate.txt).
The method is tools/kl_dense_rate.py's.

  (a) the fused kernel with its finish alone (smk_beta_dense_step_time): the H step over A and the W step over the stored
      transpose at beta = 0 (Itakura-Saito: divisions only) and at beta = 0.5 (one double-precision pow per entry), the KL step
      of kl_dense.hip on the same matrix and rank -- the kernel this one was derived from, the thing to compare with -- and the
      residual pass.  Device events around repeated launches, alternating, minimum of three windows.  The expectation for beta = 0
      is arithmetic: a step issues 1.5 x the KL step's matrix instructions (4 NQ + 32 NU against 4 NQ + 16 NU) over the same bytes.
  (b) one whole iteration of nmf_beta_dense at both betas, tol = 0.  Host clock around calls that end in a synchronise; per
      iteration = (time of 25 - time of 5) / 20, so set-up cancels.
  (c) orientation only: sklearn.decomposition.NMF(solver="mu", beta_loss="itakura-saito") on the host at 8192 x 4096, when sklearn
      imports.
Shapes: C3's (65536 x 16384, bf16, k = 32) and 8192 x 4096 at fp32 with k = 16 and k = 64; A = 0.25 + U[0, 1): strictly positive
in either storage.  Needs a GPU; nothing here falls back to the CPU.

    python tools/beta_dense_rate.py [--small] [--out profiles/beta_dense_rate.txt]
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
BETAS = (0.0, 0.5)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def step_ms(mat, which, k, beta, reps):
    ms = C.c_double(0)
    L.check(L.lib().smk_beta_dense_step_time(mat._h, which, k, C.c_double(beta), reps, C.byref(ms)), "smk_beta_dense_step_time")
    return ms.value


def kernels_alone(mat, m, n, k, ebytes, reps):
    best = {}
    for _ in range(3):
        for key in ((3, 0.0), (2, 0.0)) + tuple((which, beta) for beta in BETAS for which in (0, 1)):
            t = step_ms(mat, key[0], k, key[1], reps)
            best[key] = min(best.get(key, t), t)
    res, kl = best[(3, 0.0)], best[(2, 0.0)]
    gbytes = m * n * ebytes / 1e9
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of {reps} launches, alternating)")
    say(f"      residual pass over A        {res:8.4f} = {gbytes / res * 1e3:7.1f} GB/s of A")
    say(f"      KL step over A (kl_dense)   {kl:8.4f} = {kl / res:.2f} x the residual pass")
    for beta in BETAS:
        for which, side in ((0, "H step over A "), (1, "W step over A'")):
            t = best[(which, beta)]
            say(f"      beta = {beta:3.1f}  {side}  {t:8.4f} = {t / kl:5.2f} x the KL step, {t / res:5.2f} x the residual pass, "
                f"{gbytes / t * 1e3:7.1f} GB/s of the one read, {m * n / t / 1e6:7.1f} G entries/s")


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
    for beta in BETAS:
        it = per_iteration(lambda its: smallk_amd.nmf_beta_dense(mat, W0, H0, beta_loss=beta, tol=0.0, max_iter=its))
        say(f"  (b) k = {k}, beta = {beta}: one iteration of nmf_beta_dense {it * 1e3:.3f} ms from the host clock (two steps; no host read between checks)")


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
            NMF(k, init="custom", solver="mu", beta_loss="itakura-saito", tol=0.0, max_iter=it).fit_transform(X, W=W.copy(), H=H.copy())
    t1 = time.perf_counter(); run(1); t3 = time.perf_counter(); run(3); t = time.perf_counter()
    say(f"  (c) orientation only: sklearn.decomposition.NMF(solver='mu', beta_loss='itakura-saito') on the host, same shape, k = {k}: "
        f"{((t - t3) - (t3 - t1)) / 2 * 1e3:.0f} ms per iteration")


def shape(m, n, storage, ks, reps, with_sklearn):
    say(f"dense {m} x {n}, {storage} storage, A = 0.25 + U[0, 1)")
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32).add_(0.25)
    mat = smallk_amd.DenseMatrix.from_device(t, storage=storage)
    del t
    try:
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
