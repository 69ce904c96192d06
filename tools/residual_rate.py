#!/usr/bin/env python3
"""What the reconstruction error ||A - W H||_F costs on the device, and what it stands beside (profiles/residual_rate.txt).

Three cases on one GPU: C3's shape (65536 x 16384, bf16 storage, k = 32), C2's shape (8192 x 4096, fp32 storage, k = 16) and
the 10^6-node graph of the `s_1m` workload (sparse, k = 32).  For each:
  (r) ``A.residual(W, H)`` with the factors as torch tensors in GPU memory: host clock around the call, which ends in a
      stream synchronise -- the whole entry (workspace, factor copy, kernels, read-back).  Warm, then several windows of
      several calls each; minimum, average and maximum window.  Dense: also the kernels by themselves (launch_residual_dense on
      buffers laid out as the library lays them out, device events around `reps` launches).
  (a) the route without the feature, examples/device_nmf.py's: ``torch.linalg.norm(A.double() - W @ H)`` with its peak of
      extra device memory.  For the sparse matrix there is no such route (W H has 10^12 entries): the row says so.
  (b) the work it is held against: dense, one accurate-form pass W'A of a solver on the same matrix (SMK_NSPLIT=8,
      kernel_time(0): the same flops through the same matrix instruction); sparse, one gather product W'A
      (SparseMatrix.product(..., reps=...): the same gathers).  The expectation is (r, kernels) <= 1.3 x (b).
Needs a GPU; nothing here falls back to the CPU.

    python tools/residual_rate.py [--small] [--out profiles/residual_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("SMK_NSPLIT", "8")          # the solvers below take the accurate product form (read once per process)
os.environ.setdefault("SMK_TIMING_STRIDE", "1")   # ... and every pass of theirs is timed
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd
from smallk_amd import _lib as L

LAUNCH_DENSE = "_ZN3smk21launch_residual_denseEPKvilllPKdS3_iiPdS4_S4_S4_iP12ihipStream_t"
SCRATCH_DENSE = "_ZN3smk28residual_dense_scratch_elemsElli"
FP64_MFMA_PEAK = 78.6e12          # MI355X, fp64 matrix
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def round_up(x, m):
    return (x + m - 1) // m * m


def windows(fn, calls, nwin):
    """warm-up, then nwin windows of `calls` calls each (each call synchronises); seconds per call: min, avg, max window"""
    fn()
    fn()
    out = []
    for _ in range(nwin):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls)
    return min(out), sum(out) / len(out), max(out)


def event_windows(fn, reps, nwin):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3 / reps)
    return min(out), sum(out) / len(out), max(out)


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms (avg {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def kernels_alone(m, n, k, storage, cus):
    """launch_residual_dense by itself on the caller's stream, on buffers laid out as smk_matrix_create lays A out"""
    lib = L.lib()
    try:
        launch, elems = getattr(lib, LAUNCH_DENSE), getattr(lib, SCRATCH_DENSE)
    except AttributeError:
        return None
    launch.restype, elems.restype = C.c_int, C.c_size_t
    es = 2 if storage == "bf16" else 4
    ldA = round_up(m, 256)
    if (ldA * es) % (1 << 20) == 0:
        ldA += 128
    A = (torch.rand((round_up(n, 256), ldA), device="cuda") * 2).to(torch.bfloat16 if es == 2 else torch.float32)
    KP = 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64
    Wt = torch.rand((m, KP), dtype=torch.float64, device="cuda")
    H = torch.rand((n, KP), dtype=torch.float64, device="cuda")
    i64, vp = C.c_int64, C.c_void_p
    scratch = torch.empty(elems(i64(m), i64(n), cus), dtype=torch.float64, device="cuda")
    col_r, col_a, out2 = (torch.empty(x, dtype=torch.float64, device="cuda") for x in (n, n, 2))
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def once():
        rc = launch(vp(A.data_ptr()), L.STORE_BF16 if es == 2 else L.STORE_F32, i64(ldA), i64(m), i64(n), vp(Wt.data_ptr()), vp(H.data_ptr()),
                    KP, k, vp(scratch.data_ptr()), vp(col_r.data_ptr()), vp(col_a.data_ptr()), vp(out2.data_ptr()), cus, stream)
        assert rc == 0, rc
    return event_windows(once, 10, 5)


def dense_case(name, m, n, k, storage, alg):
    say(f"{name}: dense {m} x {n}, storage {storage}, k = {k}")
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32)
    W = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64)
    H = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float64) * (2.0 / k)
    D = smallk_amd.DenseMatrix.from_device(A, storage=storage)
    res = D.residual(W, H)
    r = windows(lambda: D.residual(W, H), 5, 5)
    say(f"  (r) A.residual(W, H), device factors, whole entry: {ms(r)}; relative error {res.relative:.6f}")
    kern = kernels_alone(m, n, k, storage, L.lib().smk_device_cu_count())
    flops = 2.0 * m * n * k
    if kern:
        say(f"  (r) its kernels alone (launch_residual_dense):    {ms(kern)}; 2 m n k = {flops / 1e12:.2f} TFLOP -> "
            f"{flops / kern[0] / 1e12:.1f} TFLOP/s = {100 * flops / kern[0] / FP64_MFMA_PEAK:.0f} % of the fp64 matrix peak; "
            f"A streamed at {m * n * (2 if storage == 'bf16' else 4) / kern[0] / 1e12:.2f} TB/s")
    else:
        say("  (r) its kernels alone: not measured (launch function not exported by this build)")
    # (a) the torch route on the stored values
    As = D.to_device(torch.float32)
    del A
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()

    def torch_route():
        return (torch.linalg.norm(As.double() - W @ H) / torch.linalg.norm(As.double())).item()
    a = windows(torch_route, 2, 3)
    peak = torch.cuda.max_memory_allocated() - base
    say(f"  (a) torch.linalg.norm(A.double() - W @ H) / norm(A.double()): {ms(a)}, {peak / 2**30:.1f} GiB of temporaries; "
        f"value {torch_route():.6f}; {a[0] / r[0]:.1f} x the entry")
    del As
    torch.cuda.empty_cache()
    # (b) one accurate-form pass W'A of a solver on the same matrix
    s = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n, k, alg, min_iter=100, max_iter=100))
    s.set_factors_device(W, H)
    form = s.product_form()[0]
    s.iterate(2)
    assert s.sync() == 0
    s.enable_timing(True)
    s.iterate(16)
    assert s.sync() == 0
    t0, c0 = s.kernel_time(0)
    b = t0 / max(c0, 1) * 1e-3
    say(f"  (b) one W'A pass of a {alg} solver, product form {form} ({s.kernel_name(0)}): {b * 1e3:9.3f} ms ({c0} launches timed)")
    if kern:
        say(f"      kernels alone / (b) = {kern[0] / b:.2f}  (expectation: <= 1.30)")
    s.close()
    D.close()
    say()


def sparse_case(k):
    import bench_sparse
    t0 = time.perf_counter()
    A = bench_sparse.make_matrix("s_1m")
    m, n = A.shape
    say(f"s_1m: sparse {m} x {n}, {A.nnz} stored entries, k = {k} (generated in {time.perf_counter() - t0:.1f} s)")
    S = smallk_amd.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    g = torch.Generator(device="cuda").manual_seed(2)
    W = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64)
    H = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float64) * (2.0 * A.nnz / (m * n) / k)
    t0 = time.perf_counter()
    res = S.residual(W, H)
    say(f"  first call (segment plan, duplicate record from the host copy of the CSC): {time.perf_counter() - t0:.2f} s")
    r = windows(lambda: S.residual(W, H), 5, 5)
    say(f"  (r) A.residual(W, H), device factors, whole entry (W'W, sampled product, quadratic forms, sums): {ms(r)}; relative error {res.relative:.6f}")
    say("  (a) the torch route cannot run: W @ H has 10^12 entries (8 TB in fp64)")
    X = np.asfortranarray(W.cpu().numpy().T)
    _, b_ms = S.product(X, reps=20)
    say(f"  (b) one gather product W'A at k = {k} (SparseMatrix.product, 20 launches): {b_ms:9.3f} ms")
    say(f"      entry / (b) = {r[0] * 1e3 / b_ms:.2f}  (expectation for the kernels: <= 1.30; the entry also copies the factors and forms W'W)")
    S.close()
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="C2's shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}; times are the minimum window unless noted (5 windows after two warm-up calls)")
    dense_case("C2", 8192, 4096, 16, "f32", "BPP")
    if not args.small:
        dense_case("C3", 65536, 16384, 32, "bf16", "HALS")
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        sparse_case(32)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
