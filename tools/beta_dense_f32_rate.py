#!/usr/bin/env python3
"""What the fp32 form of the dense KL and Itakura-Saito half-iterations costs beside the fp64 form (profiles/beta_dense_f32_rate.txt;
DESIGN.md 23).  The method is tools/beta_dense_rate.py's.

  (a) kernels alone with their finish (smk_beta_dense_f32_step_time): the fp32 H step over A and W step over the stored transpose,
      the fp64 step of the same beta on the same matrix and rank -- the thing to compare with --, and the residual pass.  Device
      events around repeated launches, the forms alternating, the minimum of three windows of 20 launches.  Beside them the two
      floors: the fp32 matrix rate for 2 (2 m n k) flops at beta = 1 and 3 (2 m n k) at beta = 0, and one read of A at the copy rate
      (a device-to-device copy of the same bytes, timed here; it reads and writes, so its time is halved).
  (b) one whole iteration with precision="fp32" and "fp64", tol = 0.  Host clock around calls that end in a synchronise; per
      iteration = (time of 25 - time of 5) / 20, so set-up cancels.
Shapes: C3's (65536 x 16384, bf16, k = 32) and 8192 x 4096 at fp32 with k = 16 and k = 64; A = 0.25 + U[0, 1): strictly positive
in either storage.  Needs a GPU; nothing here falls back to the CPU.

    python tools/beta_dense_f32_rate.py [--small] [--out profiles/beta_dense_f32_rate.txt]
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
BETAS = (1.0, 0.0)
F32_MATRIX_TFLOPS = 157.3          # MI355X, fp32 matrix, the data sheet's peak
REPS = 20


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def step_ms(mat, which, k, beta, reps):
    ms = C.c_double(0)
    L.check(L.lib().smk_beta_dense_f32_step_time(mat._h, which, k, C.c_double(beta), reps, C.byref(ms)), "smk_beta_dense_f32_step_time")
    return ms.value


def copy_ms(nbytes, reps):
    """half the time of a device-to-device copy of nbytes: the read alone at the copy rate"""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        dst.copy_(src)
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / reps / 2
        best = t if best is None else min(best, t)
    return best


def kernels_alone(mat, m, n, k, ebytes, reps):
    best = {}
    for _ in range(3):
        for key in ((3, 1.0),) + tuple((which, beta) for beta in BETAS for which in (2, 0, 1)):
            t = step_ms(mat, key[0], k, key[1], reps)
            best[key] = min(best.get(key, t), t)
    res = best[(3, 1.0)]
    gbytes = m * n * ebytes / 1e9
    read = copy_ms(m * n * ebytes, reps)
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of {reps} launches, alternating)")
    say(f"      residual pass over A          {res:8.4f} = {gbytes / res * 1e3:7.1f} GB/s of A")
    say(f"      one read of A at the copy rate {read:7.4f} = {gbytes / read * 1e3:7.1f} GB/s")
    for beta in BETAS:
        f64 = best[(2, beta)]
        floor = (2 if beta == 1.0 else 3) * 2.0 * m * n * k / (F32_MATRIX_TFLOPS * 1e12) * 1e3
        say(f"      beta = {beta:3.1f}  fp64 step over A   {f64:8.4f} = {f64 / res:5.2f} x the residual pass;  fp32 matrix floor {floor:.4f}")
        for which, side in ((0, "fp32 H step over A "), (1, "fp32 W step over A'")):
            t = best[(which, beta)]
            say(f"      beta = {beta:3.1f}  {side} {t:8.4f} = {f64 / t:5.2f} x faster than the fp64 step, {t / res:5.2f} x the residual pass, "
                f"{gbytes / t * 1e3:7.1f} GB/s of the one read, {t / max(floor, read):5.2f} x the larger floor")


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
        its = {p: per_iteration(lambda its: smallk_amd.nmf_beta_dense(mat, W0, H0, beta_loss=beta, tol=0.0, max_iter=its, precision=p))
               for p in ("fp32", "fp64")}
        say(f"  (b) k = {k}, beta = {beta}: one iteration {its['fp32'] * 1e3:.3f} ms with precision='fp32', {its['fp64'] * 1e3:.3f} ms with 'fp64' "
            f"(host clock; two steps, at beta = 1 two row-sum launches)")


def shape(m, n, storage, ks, reps):
    say(f"dense {m} x {n}, {storage} storage, A = 0.25 + U[0, 1)")
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32).add_(0.25)
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
        shape(65536, 16384, "bf16", (32,), REPS)
    shape(8192, 4096, "f32", (16, 64), REPS)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
