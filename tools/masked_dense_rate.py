#!/usr/bin/env python3
"""What the masked dense half-iterations and an iteration cost on the device (profiles/masked_dense_rate.txt).  The
method is tools/beta_dense_rate.py's.

  (a) the fused kernel with its finish alone (smk_masked_dense_step_time): the H step over A and the W step over the stored
      transpose at beta = 2, 1, 0, and the beta = 0 step of beta_dense.hip over the same A at the same rank -- the kernel this one
      was derived from, timed in the same process.  Device events around repeated launches, alternating, minimum of three windows.
      The expectation is arithmetic: beta = 0 and beta = 1 issue the matrix instructions of that step (4 NQ + 32 NU) plus selects,
      beta = 2 the same without a division; the fraction missing changes neither the bytes nor the instructions.
  (b) one whole iteration of nmf_masked_dense per beta, tol = 0.  Host clock around calls that end in a synchronise; per
      iteration = (time of 25 - time of 5) / 20, so set-up (the look at the stored values included) cancels.
Shapes: C3's (65536 x 16384, bf16, k = 32) and 8192 x 4096 at fp32 with k = 16 and k = 64; A = 0.25 + U[0, 1) with 0 %, 40 % and
90 % of the entries replaced by NaN at random.  Needs a GPU; nothing here falls back to the CPU.

    python tools/masked_dense_rate.py [--small] [--out profiles/masked_dense_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import smallk_amd
from smallk_amd import _lib as L

lines = []
BETAS = (2, 1, 0)
MISSING = (0.0, 0.4, 0.9)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def step_ms(mat, which, k, beta, reps):
    ms = C.c_double(0)
    L.check(L.lib().smk_masked_dense_step_time(mat._h, which, k, C.c_double(beta), reps, C.byref(ms)), "smk_masked_dense_step_time")
    return ms.value


def kernels_alone(mat, m, n, k, ebytes, reps):
    best = {}
    for _ in range(3):
        for key in ((2, 0),) + tuple((which, beta) for beta in BETAS for which in (0, 1)):
            t = step_ms(mat, key[0], k, key[1], reps)
            best[key] = min(best.get(key, t), t)
    base = best[(2, 0)]
    gbytes = m * n * ebytes / 1e9
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of {reps} launches, alternating)")
    say(f"      beta = 0 step of beta_dense.hip over A   {base:8.4f} = {gbytes / base * 1e3:7.1f} GB/s of A")
    for beta in BETAS:
        for which, side in ((0, "H step over A "), (1, "W step over A'")):
            t = best[(which, beta)]
            say(f"      masked beta = {beta}  {side}           {t:8.4f} = {t / base:5.2f} x that step, {gbytes / t * 1e3:7.1f} GB/s of the one read")


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
        it = per_iteration(lambda its: smallk_amd.nmf_masked_dense(mat, W0, H0, beta_loss=beta, tol=0.0, max_iter=its))
        say(f"  (b) k = {k}, beta = {beta}: one iteration of nmf_masked_dense {it * 1e3:.3f} ms from the host clock (two steps; no host read between checks)")


def shape(m, n, storage, ks, reps):
    for missing in MISSING:
        say(f"dense {m} x {n}, {storage} storage, A = 0.25 + U[0, 1), {missing:.0%} of the entries NaN")
        g = torch.Generator(device="cuda").manual_seed(7)
        t = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32).add_(0.25)
        if missing:
            t.masked_fill_(torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32) < missing, float("nan"))
        mat = smallk_amd.DenseMatrix.from_device(t, storage=storage)
        del t
        try:
            for k in ks:
                kernels_alone(mat, m, n, k, 2 if storage == "bf16" else 4, reps)
                iteration(mat, m, n, k)
        finally:
            mat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the 8192 x 4096 shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.small:
        shape(65536, 16384, "bf16", (32,), 5)
    shape(8192, 4096, "f32", (16, 64), 20)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
