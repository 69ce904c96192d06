#!/usr/bin/env python3
"""What the fp32 form of the masked dense half-iterations costs beside the fp64 form (profiles/masked_dense_f32_rate.txt;
DESIGN.md 25).  The method is tools/masked_dense_rate.py's.

  (a) kernels alone with their finish (smk_masked_dense_f32_step_time): the fp32 H step over A and W step over the stored
      transpose at beta = 2, 1, 0, and the fp64 masked step of the same beta on the same matrix and rank -- the thing to compare
      with --, timed in the same process.  Device events around repeated launches, the forms alternating, the minimum of three
      windows; the largest window over the smallest is printed as the spread.  At beta = 1 and 0 the unmasked fp32 step of
      beta_dense_f32.hip (smk_beta_dense_f32_step_time) on the same bytes stands beside them, where the matrix has no NaN.
  (b) one whole iteration with precision="fp32" and "fp64", tol = 0.  Host clock around calls that end in a synchronise; per
      iteration = (time of 25 - time of 5) / 20, so set-up (the look at the stored values included) cancels.
Shapes: C3's (65536 x 16384, bf16, k = 32) and 8192 x 4096 at fp32 with k = 16 and k = 64; A = 0.25 + U[0, 1) with 0 % and 40 % of
the entries replaced by NaN at random.  Needs a GPU; nothing here falls back to the CPU.

    python tools/masked_dense_f32_rate.py [--small] [--out profiles/masked_dense_f32_rate.txt]
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
MISSING = (0.0, 0.4)


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def step_ms(entry, mat, which, k, beta, reps):
    ms = C.c_double(0)
    L.check(getattr(L.lib(), entry)(mat._h, which, k, C.c_double(beta), reps, C.byref(ms)), entry)
    return ms.value


def kernels_alone(mat, m, n, k, ebytes, reps, unmasked):
    keys = [("smk_masked_dense_f32_step_time", which, beta) for beta in BETAS for which in (2, 0, 1)]
    if unmasked:
        keys += [("smk_beta_dense_f32_step_time", 0, beta) for beta in (1, 0)]
    seen = {key: [] for key in keys}
    for _ in range(3):
        for key in keys:
            seen[key].append(step_ms(key[0], mat, key[1], k, key[2], reps))
    best = {key: min(v) for key, v in seen.items()}
    spread = max(max(v) / min(v) for v in seen.values())
    gbytes = m * n * ebytes / 1e9
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of {reps} launches, alternating; largest window / smallest <= {spread:.3f})")
    for beta in BETAS:
        f64 = best[("smk_masked_dense_f32_step_time", 2, beta)]
        say(f"      beta = {beta}  fp64 masked step over A {f64:8.4f} = {gbytes / f64 * 1e3:7.1f} GB/s of A")
        for which, side in ((0, "fp32 H step over A "), (1, "fp32 W step over A'")):
            t = best[("smk_masked_dense_f32_step_time", which, beta)]
            line = f"      beta = {beta}  {side}    {t:8.4f} = {f64 / t:5.2f} x faster than the fp64 masked step, {gbytes / t * 1e3:7.1f} GB/s of the one read"
            if unmasked and beta != 2 and which == 0:
                u = best[("smk_beta_dense_f32_step_time", 0, beta)]
                line += f", {t / u:5.2f} x the unmasked fp32 step ({u:.4f})"
            say(line)


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
        its = {p: per_iteration(lambda its: smallk_amd.nmf_masked_dense(mat, W0, H0, beta_loss=beta, tol=0.0, max_iter=its, precision=p))
               for p in ("fp32", "fp64")}
        say(f"  (b) k = {k}, beta = {beta}: one iteration {its['fp32'] * 1e3:.3f} ms with precision='fp32', {its['fp64'] * 1e3:.3f} ms with 'fp64' (host clock; two steps)")


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
                kernels_alone(mat, m, n, k, 2 if storage == "bf16" else 4, reps, unmasked=not missing)
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
        shape(65536, 16384, "bf16", (32,), 10)
    shape(8192, 4096, "f32", (16, 64), 20)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
