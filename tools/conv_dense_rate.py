#!/usr/bin/env python3
"""What a half-iteration of convolutive NMF costs on the device (profiles/conv_dense_rate.txt).  The method is
tools/beta_dense_rate.py's: device events around repeated launches (smk_conv_dense_step_time), alternating with the yardstick,
minimum of three windows.

The yardstick is the existing plain step of nmf_beta_dense at rank T k on the same matrix (smk_beta_dense_step_time, beta = 0;
smk_kl_dense_step_time at beta = 1): the same product and the same second contractions for beta = 0, with the T-times-larger slab of
the factor in LDS and no shift-add.  At beta = 1 the plain KL step takes its denominators from factor row sums and issues half the
second contractions, so there the ratio also carries the price of the uniform second contraction.
Shapes: 65536 x 16384 bf16 and 8192 x 4096 fp32, (k, T) = (8, 4), (16, 4), (16, 8); A = 0.25 + U[0, 1).  Needs a GPU.

    python tools/conv_dense_rate.py [--small] [--out profiles/conv_dense_rate.txt]
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
CASES = ((8, 4), (16, 4), (16, 8))


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def conv_ms(mat, which, k, T, beta, reps):
    ms = C.c_double(0)
    L.check(L.lib().smk_conv_dense_step_time(mat._h, which, k, T, C.c_double(beta), reps, C.byref(ms)), "smk_conv_dense_step_time")
    return ms.value


def plain_ms(mat, which, k, beta, reps):
    ms = C.c_double(0)
    if beta == 0:
        L.check(L.lib().smk_beta_dense_step_time(mat._h, which, k, C.c_double(0.0), reps, C.byref(ms)), "smk_beta_dense_step_time")
    else:
        L.check(L.lib().smk_kl_dense_step_time(mat._h, which, k, reps, C.byref(ms)), "smk_kl_dense_step_time")
    return ms.value


def shape(m, n, storage, reps):
    say(f"dense {m} x {n}, {storage} storage, A = 0.25 + U[0, 1); ms, minimum of three windows of {reps} launches, alternating")
    g = torch.Generator(device="cuda").manual_seed(7)
    t = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32).add_(0.25)
    mat = smallk_amd.DenseMatrix.from_device(t, storage=storage)
    del t
    gbytes = m * n * (2 if storage == "bf16" else 4) / 1e9
    try:
        for k, T in CASES:
            for beta in (0, 1):
                best = {}
                for _ in range(3):
                    for which in (0, 1):
                        for key, ms in ((("conv", which), conv_ms(mat, which, k, T, beta, reps)), (("plain", which), plain_ms(mat, which, k * T, beta, reps))):
                            best[key] = min(best.get(key, ms), ms)
                for which, side in ((0, "H step over A "), (1, "W step over A'")):
                    c, p = best[("conv", which)], best[("plain", which)]
                    say(f"  k = {k:2d}, T = {T}, beta = {beta}  {side}  convolutive {c:8.4f} ({gbytes / c * 1e3:7.1f} GB/s of the one read)   "
                        f"plain step at rank {k * T:3d} {p:8.4f}   ratio {c / p:5.2f}")
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
        shape(65536, 16384, "bf16", 5)
    shape(8192, 4096, "f32", 50)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
