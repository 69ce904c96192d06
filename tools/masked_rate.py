#!/usr/bin/env python3
"""What the masked coordinate-descent sweeps and an iteration of nmf_masked cost on the device (profiles/masked_rate.txt).

  (a) the H sweep and the W sweep alone (smk_masked_step_time) against the KL half-step of the same side (smk_kl_step_time: the same
      bytes, one row of the other factor per stored entry, without the k-step chain) and against the plain gather launch_spmm_seg on
      the same plan.  Device events around repeated launches, alternating, minimum of three windows.
  (b) one iteration: nmf_masked beside nmf_cd and nmf_kl on the same matrix, tol = 0.  Host clock around calls that end in a
      synchronise; per iteration = (time of 25 - time of 5) / 20, so set-up cancels.
Shapes: the s_reuters shape (sparse 12411 x 7984) at k = 32 and the 10^6-column community graph of s_1m at k = 16, 32 and 64.  Needs a
GPU; nothing here falls back to the CPU.

    python tools/masked_rate.py [--small] [--out profiles/masked_rate.txt]
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


def step_ms(entry, mat, which, k, reps=20):
    ms = C.c_double(0)
    L.check(getattr(L.lib(), entry)(mat._h, which, k, reps, C.byref(ms)), entry)
    return ms.value


def kernels_alone(mat, k):
    runs = {"sweep H": ("smk_masked_step_time", 0), "sweep W": ("smk_masked_step_time", 1), "kl H": ("smk_kl_step_time", 0),
            "kl W": ("smk_kl_step_time", 1), "gather H": ("smk_kl_step_time", 2), "gather W": ("smk_kl_step_time", 3),
            "kl H (masked entry)": ("smk_masked_step_time", 2), "gather H (masked entry)": ("smk_masked_step_time", 3)}
    best = {}
    for _ in range(3):
        for name, (entry, which) in runs.items():
            t = step_ms(entry, mat, which, k)
            best[name] = min(best.get(name, t), t)
    say(f"  (a) k = {k}, kernels alone (ms; minimum of three windows of 20 launches, alternating)")
    for side, what in (("H", "CSC(A) "), ("W", "CSC(A')")):
        s, q, g = best[f"sweep {side}"], best[f"kl {side}"], best[f"gather {side}"]
        say(f"      {side} side, {what}: masked sweep {s:8.4f} | KL half-step {q:8.4f} | plain gather {g:8.4f} | sweep = {s / q:.2f} x KL, {s / g:.2f} x the gather")
    say(f"      smk_masked_step_time's own 2 / 3 (H side): KL half-step {best['kl H (masked entry)']:8.4f} | plain gather {best['gather H (masked entry)']:8.4f}")


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
    mk = per_iteration(lambda it: smallk_amd.nmf_masked(mat, W0, H0, tol=0.0, max_iter=it))
    cd = per_iteration(lambda it: smallk_amd.nmf_cd(mat, W0, H0, tol=0.0, max_iter=it))
    kl = per_iteration(lambda it: smallk_amd.nmf_kl(mat, W0, H0, tol=0.0, max_iter=it))
    say(f"  (b) k = {k}: one iteration of nmf_masked {mk * 1e3:.3f} ms | nmf_cd {cd * 1e3:.3f} ms | nmf_kl {kl * 1e3:.3f} ms | masked / cd = {mk / cd:.2f}, "
        f"masked / KL = {mk / kl:.2f}")


def shape(name, ks):
    import bench_sparse
    A = bench_sparse.make_matrix(name).tocsc()
    A.sum_duplicates()
    A.data = np.abs(A.data)
    m, n = A.shape
    cols, rows = np.diff(A.indptr), np.bincount(A.indices, minlength=m)
    say(f"{name}: sparse {m} x {n}, {A.nnz} stored entries; longest column {cols.max()} entries, longest row {rows.max()}; columns / rows longer than "
        f"a segment of 64: {(cols > 64).sum()} / {(rows > 64).sum()}")
    S = smallk_amd.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    try:
        for k in ks:
            kernels_alone(S, k)
            iterations(S, m, n, k)
    finally:
        S.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the s_reuters shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    shape("s_reuters", [32])
    if not args.small:
        shape("s_1m", [32, 16, 64])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
