#!/usr/bin/env python3
"""What the second stream costs: the weighted dense half-iterations beside the masked ones (profiles/weighted_dense_rate.txt;
DESIGN.md 26).  The method is tools/masked_dense_f32_rate.py's.

Kernels alone with their finish: the weighted H step over A and V and W step over the stored transposes
(smk_weighted_dense_step_time) at beta = 2, 1, 0, the fp32 masked step (the same entry, which = 2) and the fp64 masked step
(smk_masked_dense_f32_step_time, which = 2) of the same beta on the same resident A and rank, timed in the same process.  Device
events around repeated launches, the forms alternating, the minimum of three windows; the largest window over the smallest is
printed as the spread.  Beside them the time of two reads of A at the copy rate: a device-to-device copy of A moves its bytes
twice (one read, one write), so its time stands for it.
Shapes: 65536 x 16384, bf16, k = 32, and 8192 x 4096 at fp32 with k = 16 and k = 64; A = 0.25 + U[0, 1), V = 0.25 + U[0, 1) with
20 % zeros.  Needs a GPU; nothing here falls back to the CPU.

    python tools/weighted_dense_rate.py [--small] [--out profiles/weighted_dense_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import smallk_amd
from smallk_amd import _lib as L

lines = []
BETAS = (2, 1, 0)
WINDOW = 20


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def weighted_ms(mat, wts, which, k, beta):
    ms = C.c_double(0)
    L.check(L.lib().smk_weighted_dense_step_time(mat._h, wts._h, which, k, C.c_double(beta), WINDOW, C.byref(ms)), "smk_weighted_dense_step_time")
    return ms.value


def fp64_ms(mat, k, beta):
    ms = C.c_double(0)
    L.check(L.lib().smk_masked_dense_f32_step_time(mat._h, 2, k, C.c_double(beta), WINDOW, C.byref(ms)), "smk_masked_dense_f32_step_time")
    return ms.value


def copy_ms(t):
    """a device-to-device copy of t: its bytes once read and once written"""
    out = torch.empty_like(t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        out.copy_(t)
        e0.record()
        for _ in range(WINDOW):
            out.copy_(t)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / WINDOW)
    return best


def kernels_alone(mat, wts, k, two_reads):
    forms = {"fp64": lambda beta: fp64_ms(mat, k, beta), "masked": lambda beta: weighted_ms(mat, wts, 2, k, beta),
             "H": lambda beta: weighted_ms(mat, wts, 0, k, beta), "W": lambda beta: weighted_ms(mat, wts, 1, k, beta)}
    seen = {(f, beta): [] for beta in BETAS for f in forms}
    for _ in range(3):
        for key in seen:
            seen[key].append(forms[key[0]](key[1]))
    best = {key: min(v) for key, v in seen.items()}
    spread = max(max(v) / min(v) for v in seen.values())
    say(f"  k = {k}, kernels with their finish (ms; minimum of three windows of {WINDOW} launches, alternating; largest window / smallest <= {spread:.3f}); "
        f"two reads of A at the copy rate {two_reads:.4f}")
    for beta in BETAS:
        f64, mk = best[("fp64", beta)], best[("masked", beta)]
        say(f"      beta = {beta}  fp64 masked step {f64:8.4f}   fp32 masked step {mk:8.4f}")
        for f, side in (("H", "weighted H step over A, V  "), ("W", "weighted W step over A', V'")):
            t = best[(f, beta)]
            say(f"      beta = {beta}  {side} {t:8.4f} = {f64 / t:5.2f} x faster than the fp64 masked step, {t / mk:5.2f} x the fp32 masked step, "
                f"{t / two_reads:5.2f} x two reads")


def shape(m, n, storage, ks):
    say(f"dense {m} x {n}, {storage} storage, A = 0.25 + U[0, 1), V = 0.25 + U[0, 1) with 20 % zeros")
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32).add_(0.25)
    mat = smallk_amd.DenseMatrix.from_device(t, storage=storage)
    t.uniform_(0.25, 1.25, generator=g).masked_fill_(torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32) < 0.2, 0.0)
    wts = smallk_amd.DenseMatrix.from_device(t, storage=storage)
    two_reads = copy_ms(t.to(torch.bfloat16) if storage == "bf16" else t)
    del t
    try:
        for k in ks:
            kernels_alone(mat, wts, k, two_reads)
    finally:
        mat.close()
        wts.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the 8192 x 4096 shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    if not args.small:
        shape(65536, 16384, "bf16", (32,))
    shape(8192, 4096, "f32", (16, 64))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
