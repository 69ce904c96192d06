#!/usr/bin/env python3
"""What the coordinate-descent sweep and a coordinate-descent iteration cost on the device (profiles/cd_rate.txt).

  (a) the sweep alone, device events around repeated launches (smk_cd_sweep_time), k = 16 / 32 / 64 / 128 on 10^6 columns: the
      shipped column-tile form, the maintained-gradient form and launch_hals_sweep (untouched by this feature: the yardstick),
      alternating, minimum of three windows; the two forms' violations are compared.
  (r) the sweep reading S partial products itself against launch_reduce_partials + a sweep on the reduced product, on C3's two
      factor lengths.
  (b) one iteration: nmf_cd on C3's shape (65536 x 16384, bf16 storage, k = 32) and on the s_reuters shape (sparse 12411 x 7984,
      k = 32) against a HALS iteration of NmfSolver on the same matrix under SMK_NSPLIT=8 (the same two products).  Host clock
      around calls that end in a synchronise; per iteration = (time of 25 - time of 5) / 20, so set-up cancels.
  (c) orientation only: sklearn.decomposition.NMF(solver="cd") on the host for the s_reuters shape, when sklearn imports.
Needs a GPU; nothing here falls back to the CPU.

    python tools/cd_rate.py [--small] [--out profiles/cd_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("SMK_NSPLIT", "8")          # the HALS yardstick takes the accurate product form (read per solver)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd
from smallk_amd import _lib as L

lines = []
NAMES = {0: "cd sweep", 1: "cd sweep, maintained gradient", 2: "hals sweep", 3: "reduce partials"}


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def sweep_ms(which, k, N, slabs=1, reps=20):
    ms, chk = C.c_double(0), C.c_double(0)
    L.check(L.lib().smk_cd_sweep_time(which, k, N, slabs, reps, C.byref(ms), C.byref(chk)), "smk_cd_sweep_time")
    return ms.value, chk.value


def sweeps_alone(N, ks):
    say(f"(a) one sweep over {N} columns, kernels alone (ms; minimum of three windows of 20 launches, alternating)")
    for k in ks:
        best, chk = {}, {}
        for _ in range(3):
            for which in (2, 0, 1):
                t, c = sweep_ms(which, k, N)
                best[which] = min(best.get(which, t), t)
                chk[which] = c
        kp = 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
        gbs = 3.0 * N * kp * 8 / (best[0] * 1e-3) / 1e9            # X read and written, R read
        say(f"  k = {k:3d}: hals {best[2]:8.3f} | cd {best[0]:8.3f} ({best[0] / best[2]:.2f} x hals, {gbs:.0f} GB/s) | maintained gradient "
            f"{best[1]:8.3f} ({best[1] / best[0]:.2f} x cd); violations agree to {abs(chk[0] - chk[1]) / chk[0]:.1e}")


def partials_compare(k, lengths, slab_counts):
    say(f"(r) k = {k}: the sweep reading S partial products itself | reduction + sweep on the reduced product (ms)")
    for N in lengths:
        for S in slab_counts:
            direct = min(sweep_ms(0, k, N, S)[0] for _ in range(3))
            red = min(sweep_ms(3, k, N, S)[0] for _ in range(3))
            one = min(sweep_ms(0, k, N, 1)[0] for _ in range(3))
            say(f"  {N:6d} columns, S = {S}: {direct:.4f} | {red:.4f} + {one:.4f} = {red + one:.4f}")


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_iteration(run, lo=5, hi=25, n=3):
    run(lo)
    return min((clocked(lambda: run(hi)) - clocked(lambda: run(lo))) / (hi - lo) for _ in range(n))


def iteration_case(name, mat, m, n, k):
    g = torch.Generator(device="cuda").manual_seed(2)
    W0 = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64)
    H0 = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float64) * (2.0 / k)
    cd = per_iteration(lambda it: smallk_amd.nmf_cd(mat, W0, H0, tol=0.0, max_iter=it))
    s = smallk_amd.NmfSolver(mat, smallk_amd.make_options(m, n, k, "HALS", min_iter=1000, max_iter=1000))
    s.set_factors_device(W0, H0)

    def hals(it):
        s.iterate(it)
        assert s.sync() == 0
    hl = per_iteration(hals)
    form = s.product_form()[0]
    s.close()
    say(f"(b) {name}, k = {k}: one cd iteration {cd * 1e3:.3f} ms (the violation read by the host every iteration) | one HALS iteration "
        f"(product form {form}, no stopping-rule check) {hl * 1e3:.3f} ms | cd / HALS = {cd / hl:.2f}")
    return W0, H0


def sklearn_case(A, k):
    try:
        from sklearn.decomposition import NMF
    except Exception as e:          # noqa: BLE001
        say(f"(c) sklearn does not import here ({type(e).__name__}): omitted")
        return
    import warnings
    X = A.T.tocsr()
    rng = np.random.default_rng(2)
    W, H = rng.random((X.shape[0], k)) * (2.0 / k), rng.random((k, X.shape[1]))

    def run(it):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            NMF(k, init="custom", solver="cd", tol=0.0, max_iter=it, shuffle=False).fit_transform(X, W=W.copy(), H=H.copy())
    t2 = time.perf_counter(); run(2); t6 = time.perf_counter(); run(6); t = time.perf_counter()
    say(f"(c) orientation only: sklearn.decomposition.NMF(solver='cd') on the host, same shape: {((t - t6) - (t6 - t2)) / 4 * 1e3:.1f} ms per iteration")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="short factors and the sparse case only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    sweeps_alone(100_000 if args.small else 1_000_000, (16, 32, 64, 128))
    partials_compare(32, (16384, 65536), (2, 4, 8))
    if not args.small:
        m, n, k = 65536, 16384, 32
        g = torch.Generator(device="cuda").manual_seed(1)
        A = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32)
        D = smallk_amd.DenseMatrix.from_device(A, storage="bf16")
        del A
        iteration_case(f"C3's shape (dense {m} x {n}, bf16 storage)", D, m, n, k)
        D.close()
    import bench_sparse
    A = bench_sparse.make_matrix("s_reuters")
    m, n = A.shape
    S = smallk_amd.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    iteration_case(f"s_reuters shape (sparse {m} x {n}, {A.nnz} stored entries)", S, m, n, 32)
    S.close()
    sklearn_case(A, 32)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
