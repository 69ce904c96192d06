#!/usr/bin/env python3
"""What the NNDSVD start costs on the device and what it consists of (profiles/svd_rate.txt).

Three cases on one GPU: C3's shape (65536 x 16384, bf16 storage, k = 32), C2's shape (8192 x 4096, fp32 storage, k = 16) and
the 10^6-node graph of the `s_1m` workload (sparse, k = 32), each with q = 0 and q = 2 power iterations.  Per case:
  (n) ``A.nndsvd(k)``: host clock around the call (it ends in a stream synchronise); warm, minimum of five calls;
  (p) the 2 q + 2 passes over A it contains, timed alone: dense, the accurate-form passes of a solver of rank l = k + 8 on the
      same matrix (SMK_NSPLIT=8, enable_timing / kernel_time: they exist without this feature, so they are the yardstick);
      sparse, the gather products of SparseMatrix.product at rank l;
  (t) the tall-skinny apply kernel alone on factors of the entry's shapes (device events around repeated launches), times
      the number of applies of the entry;
  (h) the Gram matrices that went to the host and the time their eigendecompositions took (smk_svd_last_profile);
  (o) dense only, for orientation (it is fp32): torch.svd_lowrank on the fp32 tensor with the same l and q.
Expectation, not a gate: (n) <= 1.3 x (p) on the dense cases.
Last, on planted data at C2's shape: the relative residual after 0, 5, 10 and 20 BPP iterations from the NNDSVD start and
from the uniform start.  Needs a GPU; nothing here falls back to the CPU.

    python tools/svd_rate.py [--small] [--out profiles/svd_rate.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("SMK_NSPLIT", "8")          # the solvers below take the accurate product form (read once per process)
os.environ.setdefault("SMK_TIMING_STRIDE", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import smallk_amd
from smallk_amd import _lib as L

LAUNCH_APPLY = "_ZN3smk16launch_svd_applyEPKdPdilS1_iiiiP12ihipStream_t"
LAUNCH_APPLY_GRAM = "_ZN3smk21launch_svd_apply_gramEPKdPdilS1_iiiS2_PiiP12ihipStream_t"
LAUNCH_GRAM = "_ZN3smk11launch_gramEPKdilPdS2_iP12ihipStream_tS2_S2_d"
LAUNCH_GRAM_REDUCE = "_ZN3smk18launch_gram_reduceEPKdiiPdP12ihipStream_tS2_S2_d"
APPLY_GRAM_BLOCKS = "_ZN3smk21svd_apply_gram_blocksEili"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def min_of(fn, n=5):
    fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return min(out)


def kp_of(l):
    return 8 if l <= 8 else 16 if l <= 16 else 32 if l <= 32 else 64 if l <= 64 else 128


def apply_alone(N, l):
    """launch_svd_apply in place on a KP x N factor: seconds per launch, minimum of five windows of ten launches"""
    launch = getattr(L.lib(), LAUNCH_APPLY)
    launch.restype = C.c_int
    KP = kp_of(l)
    X = torch.rand((N, KP), dtype=torch.float64, device="cuda")
    M = torch.eye(l, dtype=torch.float64, device="cuda")
    vp, stream = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cus = L.lib().smk_device_cu_count()

    def once():
        rc = launch(vp(X.data_ptr()), vp(X.data_ptr()), KP, C.c_int64(N), vp(M.data_ptr()), l, l, l, cus, stream)
        assert rc == 0, rc
    once()
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            once()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) * 1e-3 / 10
        best = t if best is None else min(best, t)
    return best, 2.0 * N * KP * 8 / best


def event_min(once, reps=10, nwin=5):
    once()
    torch.cuda.synchronize()
    best = None
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            once()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) * 1e-3 / reps
        best = t if best is None else min(best, t)
    return best


def fused_compare(N, l):
    """one orthonormalisation round's apply + the Gram matrix of its result, kernels alone: the two launches apart (the plain
    apply, then launch_gram reading the factor again) against the fused apply that leaves Gram partials + their reduction"""
    lib = L.lib()
    KP = kp_of(l)
    blocks = getattr(lib, APPLY_GRAM_BLOCKS)
    blocks.restype = C.c_int
    cus = lib.smk_device_cu_count()
    nb = blocks(KP, C.c_int64(N), cus)
    if nb < 1:
        return None
    apply_, fused, gram, reduce_ = (getattr(lib, x) for x in (LAUNCH_APPLY, LAUNCH_APPLY_GRAM, LAUNCH_GRAM, LAUNCH_GRAM_REDUCE))
    for f in (apply_, fused, gram, reduce_):
        f.restype = C.c_int
    X = torch.rand((N, KP), dtype=torch.float64, device="cuda")
    M = torch.eye(l, dtype=torch.float64, device="cuda")
    G = torch.empty(KP * KP, dtype=torch.float64, device="cuda")
    Gp = torch.empty(max(nb, 256) * KP * KP + 8, dtype=torch.float64, device="cuda")
    vp, stream, n64 = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_int64(N)
    nblk = C.c_int(0)
    one = C.c_double(1.0)

    def apart():
        assert apply_(vp(X.data_ptr()), vp(X.data_ptr()), KP, n64, vp(M.data_ptr()), l, l, l, cus, stream) == 0
        assert gram(vp(X.data_ptr()), l, n64, vp(G.data_ptr()), vp(Gp.data_ptr()), 256, stream, None, None, one) == 0

    def together():
        assert fused(vp(X.data_ptr()), vp(X.data_ptr()), KP, n64, vp(M.data_ptr()), l, l, l, vp(Gp.data_ptr()), C.byref(nblk), cus, stream) == 0
        assert reduce_(vp(Gp.data_ptr()), nblk.value, l, vp(G.data_ptr()), stream, None, None, one) == 0
    apart()
    Ga = G.clone()
    together()
    dev = (G - Ga).abs().max().item() / Ga.abs().max().item()
    return event_min(apart), event_min(together), dev


def profile():
    trips, ms = C.c_int(0), C.c_double(0)
    L.lib().smk_svd_last_profile(C.byref(trips), C.byref(ms))
    return trips.value, ms.value


def report(name, mat, m, n, k, pass_m, pass_n, dense_tensor):
    """pass_m / pass_n: seconds of one pass that contracts over the rows / over the columns of A at rank l"""
    l = min(k + 8, m, n)
    ap_m, bw_m = apply_alone(m, l)
    ap_n, bw_n = apply_alone(n, l)
    say(f"  one pass at rank l = {l}: contraction over m {pass_m * 1e3:.3f} ms, over n {pass_n * 1e3:.3f} ms")
    say(f"  tall-skinny apply alone (KP = {kp_of(l)}): {m} columns {ap_m * 1e6:.1f} us ({bw_m / 1e12:.2f} TB/s read + write), "
        f"{n} columns {ap_n * 1e6:.1f} us ({bw_n / 1e12:.2f} TB/s)")
    for N in sorted({m, n}, reverse=True):
        fc = fused_compare(N, l)
        if fc:
            say(f"  apply + Gram of the result, {N} columns, kernels alone: apart {fc[0] * 1e6:.1f} us, fused apply + reduction {fc[1] * 1e6:.1f} us "
                f"(Gram matrices agree to {fc[2]:.1e})")
    for q in (0, 2):
        t = min_of(lambda: mat.nndsvd(k, power_iters=q))
        trips, host_ms = profile()
        passes = (q + 1) * (pass_m + pass_n)
        # applies: two per orth (q + 1 on m-long factors, q on n-long), then U, V and the polish of V
        applies = (2 * (q + 1) + 1) * ap_m + (2 * q + 2) * ap_n
        say(f"  q = {q}: (n) A.nndsvd(k = {k}) {t * 1e3:9.3f} ms | (p) its {2 * q + 2} passes alone {passes * 1e3:.3f} ms | "
            f"(t) its {4 * q + 5} applies alone {applies * 1e3:.3f} ms | (h) {trips} host round trips, eigendecompositions {host_ms:.3f} ms | "
            f"(n) / (p) = {t / passes:.2f}")
        if dense_tensor is not None:
            o = min_of(lambda: torch.svd_lowrank(dense_tensor, q=l, niter=q), 3)
            say(f"         (o) torch.svd_lowrank(fp32 tensor, q = {l}, niter = {q}): {o * 1e3:.3f} ms (fp32, orientation only)")


def dense_case(name, m, n, k, storage):
    say(f"{name}: dense {m} x {n}, storage {storage}, k = {k}")
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand((m, n), generator=g, device="cuda", dtype=torch.float32)
    D = smallk_amd.DenseMatrix.from_device(A, storage=storage)
    l = min(k + 8, m, n)
    s = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n, l, "HALS", min_iter=100, max_iter=100))
    s.set_factors_uniform(3, 4)
    form = s.product_form()[0]
    s.iterate(2)
    assert s.sync() == 0
    s.enable_timing(True)
    s.iterate(8)
    assert s.sync() == 0
    (t0, c0), (t1, c1) = s.kernel_time(0), s.kernel_time(1)
    say(f"  yardstick: HALS solver of rank {l}, product form {form} ({s.kernel_name(0)}), {c0} + {c1} launches timed")
    s.close()
    report(name, D, m, n, k, t0 / max(c0, 1) * 1e-3, t1 / max(c1, 1) * 1e-3, A)
    D.close()
    say()


def sparse_case(k):
    import bench_sparse
    A = bench_sparse.make_matrix("s_1m")
    m, n = A.shape
    say(f"s_1m: sparse {m} x {n}, {A.nnz} stored entries, k = {k}")
    S = smallk_amd.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    l = k + 8
    rng = np.random.default_rng(0)
    _, pm = S.product(np.asfortranarray(rng.random((l, m))), reps=10)
    _, pn = S.product(np.asfortranarray(rng.random((l, n))), transposed=True, reps=10)
    report("s_1m", S, m, n, k, pm * 1e-3, pn * 1e-3, None)
    S.close()
    say()


def starts_case(m, n, k):
    say(f"planted data at C2's shape ({m} x {n}, fp32 storage, k = {k}): relative residual after 0 / 5 / 10 / 20 BPP iterations")
    D = smallk_amd.DenseMatrix(m, n, storage="f32")
    D.fill_planted(7, k)
    for name in ("nndsvd", "uniform"):
        s = smallk_amd.NmfSolver(D, smallk_amd.make_options(m, n, k, "BPP", min_iter=100, max_iter=100))
        if name == "nndsvd":
            s.set_factors_nndsvd()
        else:
            s.set_factors_uniform(3, 4)
        out, done = [], 0
        for it in (0, 5, 10, 20):
            s.iterate(it - done)
            done = it
            out.append(s.residual().relative)
        say(f"  from {name:8s}: " + "  ".join(f"{x:.6f}" for x in out))
        s.close()
    D.close()
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="C2's shape only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    smallk_amd.initialize(0)
    say(f"device: {torch.cuda.get_device_name(0)}; warm, minimum of five")
    dense_case("C2", 8192, 4096, 16, "f32")
    starts_case(8192, 4096, 16)
    if not args.small:
        dense_case("C3", 65536, 16384, 32, "bf16")
        sparse_case(32)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
