"""Do handles give back what they allocate?  For each configuration of a fixed list: one warm create-use-destroy cycle,
trim_device_cache(), then three more cycles, each followed by trim_device_cache(); prints the bytes each trim returned.
A handle that leaks a device block returns fewer bytes than it should; the three values of a configuration must be equal,
and equal across two builds of the library.  Every block stays below the allocator's 512 MB per-block limit and the
total below its 4 GB cap, so every freed block is counted.  The count is the process's own: other users of the GPU do
not disturb it.  Each configuration runs in a child process (some need an environment switch that is read once).
usage: python tools/handle_cycle.py            all configurations, one line each
       python tools/handle_cycle.py NAME       one configuration in this process"""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def dense(m, n, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).random((m, n)))


def sparse(m, n, density=0.01, seed=2):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=density, random_state=3, format="lil", data_rvs=lambda s: rng.random(s) + 0.1)
    A[:, 0] = 1.0           # one long column and one long row: the segment plans cut them into pieces
    A[0, :] = 1.0
    return A.tocsc()


def solve(S, A, alg, k, iters=6, how="run", **opt):
    s = S.NmfSolver(A, S.make_options(A.height, A.ncols, k, alg, min_iter=iters, max_iter=iters, **opt))
    s.set_factors_uniform(11, 12)
    if how == "run":
        s.run()
    elif how == "checked":
        s.iterate_checked(iters)
    elif how == "timing":
        s.enable_timing(True)
        s.iterate(iters)
        s.sync()
        s.kernel_time(0)
    elif how == "factors":
        s.iterate(iters)
        s.factors(normalize=True)
    s.close()


def dense_case(alg, k, m=1024, n=768, how="run", single_copy=False, **opt):
    def cycle(S):
        A = S.DenseMatrix.from_host(dense(m, n), single_copy=single_copy)
        solve(S, A, alg, k, how=how, **opt)
        A.close()
    return cycle


def sparse_case(alg, k, how="run"):
    def cycle(S):
        A = S.SparseMatrix.from_scipy(sparse(3000, 2000))
        solve(S, A, alg, k, how=how)
        A.close()
    return cycle


def guard_case(S):
    A = S.DenseMatrix.from_host(dense(1024, 768))
    solve(S, A, "BPP", 16, iters=12)          # SMK_GUARD_EVERY=4: the sample is taken at iteration 4, read at 8
    A.close()


def sharded_case(S):
    m, n, k = 1024, 768, 16
    S.nmf_sharded(dense(m, n), dense(m, k, 5), dense(k, n, 6), "BPP", 2, local_stub=True, min_iter=6, max_iter=6)


def comm_case(S):
    # SMK_COMM_EMULATE_WORLD=2: rank 0 of two on a one-rank communicator, in this thread's context (the shards of
    # sharded_case run in contexts of their own, which hand their cache back when they end: it prints 0)
    m, n, k = 2048, 1536, 16
    A = S.DenseMatrix(m, n, col0=0, ncols=n // 2)
    A.fill_uniform(42)
    comm = S.Comm.init_all(1)[0]
    s = S.NmfSolver(A, S.make_options(m, n, k, "BPP", min_iter=10, max_iter=10))
    s.attach_comm(comm)
    s.set_factors(S.uniform_host(m, k, 43), S.uniform_host(k, n // 2, 44) * (2.0 / k))
    s.iterate(4)
    s.enable_timing(True)
    s.iterate_checked(4)
    s.sync()
    s.close()
    comm.close()
    A.close()


def single_copy_case(S):
    A = S.DenseMatrix.from_host(dense(1024, 768), single_copy=True)
    solve(S, A, "MU", 16)                     # runs on the single copy
    solve(S, A, "BPP", 40)                    # asks for the stored transpose
    A.close()


def product_case(S):
    A = S.SparseMatrix.from_scipy(sparse(3000, 2000))
    A.product(dense(16, 3000, 7), reps=2)
    A.product(dense(2, 2000, 8), transposed=True)
    A.close()


def subset_case(S):
    A = S.SparseMatrix.from_scipy(sparse(3000, 2000))
    tree = S.hier_nmf2(A, 3, seed=1, tol=1e-3, max_iter=50)       # a solver and a column subset per node
    del tree
    A.close()


CONFIGS = [
    ("mu_delta_fnorm",      dense_case("MU", 16, prog_est=1), {}),
    ("hals_k16",            dense_case("HALS", 16), {}),
    ("hals_k160",           dense_case("HALS", 160), {}),
    ("bpp_k16",             dense_case("BPP", 16), {}),
    ("bpp_k64",             dense_case("BPP", 64), {}),
    ("bpp_k160",            dense_case("BPP", 160), {}),
    ("rank2_dense",         dense_case("RANK2", 2), {}),
    ("rank2_sparse",        sparse_case("RANK2", 2), {}),
    ("bpp_sparse_k16",      sparse_case("BPP", 16), {}),
    ("bpp_sparse_k40",      sparse_case("BPP", 40), {}),
    ("guard_sample",        guard_case, {"SMK_GUARD_EVERY": "4"}),
    ("iterate_checked",     dense_case("BPP", 16, how="checked"), {}),
    ("iterate_checked_mu",  dense_case("MU", 24, how="checked"), {}),
    ("timing",              dense_case("BPP", 40, how="timing"), {}),
    ("timing_sparse",       sparse_case("BPP", 16, how="timing"), {}),
    ("factors_k5",          dense_case("HALS", 5, how="factors"), {}),
    ("two_shards_local",    sharded_case, {}),
    ("attach_comm_rank0of2", comm_case, {"SMK_COMM_EMULATE_WORLD": "2"}),
    ("single_copy",         single_copy_case, {}),
    ("sparse_product",      product_case, {}),
    ("hier_nmf2_sparse",    subset_case, {}),
]


def one(name):
    import smallk_amd as S
    cycle = {n: c for n, c, _ in CONFIGS}[name]
    S.initialize(0)
    cycle(S)
    S.trim_device_cache()
    got = []
    for _ in range(3):
        cycle(S)
        got.append(S.trim_device_cache())
    note = "equal" if got[0] == got[1] == got[2] else "DIFFER"
    if name == "two_shards_local":
        note += "  (NOT A MEASUREMENT: each shard runs in a context of its own, which returns its cache when it ends; attach_comm_rank0of2 covers the sharded buffers)"
    print("%-22s %12d %12d %12d  %s" % (name, got[0], got[1], got[2], note), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        one(sys.argv[1])
        sys.exit(0)
    for name, _, env in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=dict(os.environ, **env), timeout=300)
        if r.returncode != 0:           # a configuration that failed ends the run: nothing more is started on the device
            print("%s: exit status %d" % (name, r.returncode), flush=True)
            sys.exit(1)
