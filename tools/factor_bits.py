"""Same bits, same launches?  For each configuration of a fixed list: a few iterations through the Python API, then one line with
a SHA-256 of W and H (fp64 bytes), the iteration count, kernel_name(0..2) and -- where timing is on -- the launch counts of
kernel_time(0..5).  Two builds of the library that schedule the same launches on the same data print the same lines.  The list is
made so that every consumer and every reset site of the solver's hand-off record (state.h: Handoff) runs at least once: the
packing NNLS launch and its tail, the Gram ride and the inverse ride of the gather products, the inverse beside the pass, in the
pass and in the solve, the sweeps' epilogues, solver.Init after set_factors, after project(), after a fail-soft restart and after
a fired guard.  A switch that is read once per process gets a process of its own (GROUPS), each under its own time limit.
usage: python tools/factor_bits.py            all groups, one child process each
       python tools/factor_bits.py GROUP      one group in this process"""
import hashlib, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SMALL, LARGE = (512, 256), (2048, 1024)


def dense(shape, seed=1):
    return np.asfortranarray(np.random.default_rng(seed).random(shape))


def sparse(m=3000, n=2000, density=0.01):
    import scipy.sparse as sp
    rng = np.random.default_rng(2)
    A = sp.random(m, n, density=density, random_state=3, format="lil", data_rvs=lambda s: rng.random(s) + 0.1)
    A[:, 0] = 1.0           # one long column and one long row: the segment plans cut them into pieces
    A[0, :] = 1.0
    return A.tocsc()


def ill_conditioned(m=3000, n=2000, k=8, pert=0.1):
    """the planted factor with nearly collinear columns of tools/guard_case.py"""
    rng = np.random.default_rng(5)
    Wp = rng.random((m, 1)) + pert * rng.random((m, k))
    Hp = rng.random((k, n)) * (rng.random((k, n)) > 0.5)
    return np.asfortranarray(Wp @ Hp + 1e-3 * rng.random((m, n)))


def line(name, W, H, iters, names, launches=None):
    h = hashlib.sha256(np.asfortranarray(W, dtype=np.float64).tobytes(order="F"))
    h.update(np.asfortranarray(H, dtype=np.float64).tobytes(order="F"))
    text = "%-34s %s iters=%d" % (name, h.hexdigest(), iters)
    for i, n in enumerate(names):
        text += " | %d: %s" % (i, n)
    if launches is not None:
        text += " | launches " + ",".join(str(c) for c in launches)
    print(text, flush=True)


def solver_case(name, make_matrix, alg, k, how="iterate", iters=6, env=None, **opt):
    def run(S):
        old = {v: os.environ.get(v) for v in (env or {})}
        os.environ.update(env or {})            # the switches named here are read per plan / per launch
        try:
            A = make_matrix(S)
            s = S.NmfSolver(A, S.make_options(A.height, A.ncols, k, alg, min_iter=iters, max_iter=iters, **opt))
            s.set_factors_uniform(11, 12)
            launches = None
            if how == "iterate":
                s.iterate(iters)
            elif how == "checked":
                s.iterate_checked(iters)
            elif how == "run":
                s.run()
            elif how == "timing":
                s.enable_timing(True)
                s.iterate(iters)
                s.iterate_checked(iters)
                s.sync()
                launches = [s.kernel_time(w)[1] for w in range(6)]
            elif how == "project":
                s.iterate(iters // 2)
                s.project()
                s.project()
                s.iterate(iters // 2)
            elif how == "set_twice":
                s.iterate(iters // 2)
                s.set_factors_uniform(13, 14)
                s.iterate(iters // 2)
                s.set_factors(S.uniform_host(A.height, k, 15), S.uniform_host(k, A.ncols, 16) * (2.0 / k))
                s.run()
            s.sync()
            W, H = s.factors()
            form, checks, fired, _ = s.product_form()
            line(name, W, H, s.iteration_count, [s.kernel_name(w) for w in range(3)] + ["form %d guard %d/%d" % (form, fired, checks)], launches)
            s.close()
            A.close()
        finally:
            for v, x in old.items():
                if x is None:
                    os.environ.pop(v, None)
                else:
                    os.environ[v] = x
    return name, run


def D(shape, storage="f32", single_copy=False):
    return lambda S: S.DenseMatrix.from_host(dense(shape), storage=storage, single_copy=single_copy)


def Sp():
    return lambda S: S.SparseMatrix.from_scipy(sparse())


def tag(shape, storage):
    return "%dx%d_%s" % (shape[0], shape[1], storage)


def nnls_hals_case(name, make_A):
    def run(S):
        from smallk_amd.flatclust import nnls_hals
        A = make_A()
        m, n = A.shape
        rc, W, H, its = nnls_hals(A, S.uniform_host(m, 16, 21), S.uniform_host(16, n, 22), max_iter=8)
        line(name, W, H, its, ["rc %d" % rc])
    return name, run


def sharded_case(name, alg, k):
    def run(S):
        m, n = LARGE
        r = S.nmf_sharded(dense(LARGE), dense((m, k), 5), dense((k, n), 6), alg, 2, local_stub=True, min_iter=6, max_iter=6)
        line(name, r.W, r.H, r.iteration_count, ["rc %d" % r.result])
    return name, run


def single_copy_case(name):
    def run(S):
        A = S.DenseMatrix.from_host(dense(SMALL), single_copy=True)
        for alg, k in (("MU", 16), ("HALS", 16), ("BPP", 40)):          # the last one asks for the stored transpose
            s = S.NmfSolver(A, S.make_options(A.height, A.ncols, k, alg, min_iter=6, max_iter=6))
            s.set_factors_uniform(11, 12)
            s.iterate(6)
            s.sync()
            W, H = s.factors()
            line("%s_%s_k%d" % (name, alg.lower(), k), W, H, s.iteration_count, [s.kernel_name(w) for w in range(3)])
            s.close()
        A.close()
    return name, run


FP16_FORM = {"SMK_NSPLIT": "4"}         # k in (32, 64] on a matrix of at most 2^24 entries takes the accurate form by default


def dense_list(bpp_ks, hals_ks, extras):
    out = []
    for shape in (SMALL, LARGE):
        for storage in ("f32", "bf16"):
            t = tag(shape, storage)
            for k in bpp_ks:
                out.append(solver_case("bpp_k%d_%s" % (k, t), D(shape, storage), "BPP", k))
                if storage == "f32" and 16 < k <= 64:
                    out.append(solver_case("bpp_k%d_fp16_form_%s" % (k, t), D(shape), "BPP", k, how="set_twice", env=FP16_FORM))
            for k in hals_ks:
                out.append(solver_case("hals_k%d_%s" % (k, t), D(shape, storage), "HALS", k))
            if extras:
                out.append(solver_case("mu_k16_%s" % t, D(shape, storage), "MU", 16))
                out.append(solver_case("rank2_%s" % t, D(shape, storage), "RANK2", 2, how="run"))
    return out


def default_group():
    out = dense_list((8, 12, 16, 24, 32, 40, 64, 100, 192), (16, 32), True)
    for shape in (SMALL, LARGE):
        t = tag(shape, "f32")
        for k in (8, 12, 16):
            out.append(solver_case("bpp_k%d_checked_%s" % (k, t), D(shape), "BPP", k, how="checked"))
            out.append(solver_case("bpp_k%d_run_%s" % (k, t), D(shape), "BPP", k, how="run"))
            out.append(solver_case("bpp_k%d_nopack_%s" % (k, t), D(shape), "BPP", k, how="run", env={"SMK_NNLS_PACK": "0"}))
            out.append(solver_case("bpp_k%d_pack_overflow_%s" % (k, t), D(shape), "BPP", k, how="run", env={"SMK_NNLS_PACK_TEST_ANORM": "1e-6"}))
        for k in (16, 40, 64):
            out.append(solver_case("bpp_k%d_project_%s" % (k, t), D(shape), "BPP", k, how="project"))
            out.append(solver_case("bpp_k%d_set_twice_%s" % (k, t), D(shape), "BPP", k, how="set_twice"))
            out.append(solver_case("bpp_k%d_timing_%s" % (k, t), D(shape), "BPP", k, how="timing"))
        out.append(solver_case("hals_k16_run_%s" % t, D(shape), "HALS", 16, how="run"))
        out.append(solver_case("mu_k24_checked_%s" % t, D(shape), "MU", 24, how="checked"))
        out.append(solver_case("mu_k16_delta_fnorm_%s" % t, D(shape), "MU", 16, how="run", prog_est=1))
    for alg in ("BPP", "HALS", "MU"):
        for k in (12, 32):
            out.append(solver_case("sparse_%s_k%d" % (alg.lower(), k), Sp(), alg, k))
            out.append(solver_case("sparse_%s_k%d_run" % (alg.lower(), k), Sp(), alg, k, how="run"))
    out.append(solver_case("sparse_bpp_k40", Sp(), "BPP", 40))
    out.append(solver_case("sparse_bpp_k32_timing", Sp(), "BPP", 32, how="timing"))
    out.append(solver_case("sparse_bpp_k32_project", Sp(), "BPP", 32, how="project"))
    out.append(solver_case("sparse_bpp_k12_set_twice", Sp(), "BPP", 12, how="set_twice"))
    out.append(solver_case("sparse_rank2", Sp(), "RANK2", 2, how="run"))
    out.append(solver_case("sparse_rank2_iterate", Sp(), "RANK2", 2))
    out.append(single_copy_case("single_copy"))
    out.append(nnls_hals_case("nnls_hals_dense", lambda: dense(SMALL)))
    out.append(nnls_hals_case("nnls_hals_sparse", sparse))
    out.append(sharded_case("two_shards_bpp_k16", "BPP", 16))          # W row-sharded
    out.append(sharded_case("two_shards_bpp_k64", "BPP", 64))
    out.append(sharded_case("two_shards_mu_k16", "MU", 16))
    out.append(sharded_case("two_shards_hals_k16", "HALS", 16))        # W replicated
    return out


def no_inverse_ride_group():
    out = dense_list((24, 32, 40, 64), (), False)
    out.append(solver_case("sparse_bpp_k32", Sp(), "BPP", 32))
    out.append(solver_case("sparse_bpp_k40", Sp(), "BPP", 40))
    out.append(solver_case("bpp_k64_project_%s" % tag(LARGE, "f32"), D(LARGE), "BPP", 64, how="project"))
    out.append(solver_case("bpp_k64_set_twice_%s" % tag(LARGE, "f32"), D(LARGE), "BPP", 64, how="set_twice"))
    return out


def side_stream_everywhere_group():
    out = [solver_case("bpp_k%d_%s" % (k, tag(SMALL, "f32")), D(SMALL), "BPP", k, how="set_twice") for k in (24, 64)]
    out.append(solver_case("sparse_bpp_k32", Sp(), "BPP", 32, how="set_twice"))
    return out


def no_epilogue_group():
    return dense_list((), (16, 32), False)


def guard_group():
    return [solver_case("guard_fires_bpp_k8", lambda S: S.DenseMatrix.from_host(ill_conditioned()), "BPP", 8, how="run", iters=20),
            solver_case("guard_fires_bpp_k16_iterate", lambda S: S.DenseMatrix.from_host(ill_conditioned(k=16)), "BPP", 16, iters=20)]


# name -> (the read-once switches of the process, the configurations, seconds)
GROUPS = {
    "default":           ({}, default_group, 600),
    "no_inverse_ride":   ({"SMK_INV_RIDE": "0"}, no_inverse_ride_group, 300),
    "inverse_beside":    ({"SMK_INV_RIDE": "0", "SMK_INV_STREAM": "1"}, side_stream_everywhere_group, 120),
    "no_hals_epilogue":  ({"SMK_HALS_EPILOGUE": "0"}, no_epilogue_group, 120),
    "guard_every_4":     ({"SMK_GUARD_EVERY": "4"}, guard_group, 120),
}


def one(group):
    import smallk_amd as S
    S.initialize(0)
    print("# group %s" % group, flush=True)
    for name, run in GROUPS[group][1]():
        run(S)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        one(sys.argv[1])
        sys.exit(0)
    for group, (env, _, seconds) in GROUPS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=dict(os.environ, **env), timeout=seconds)
        if r.returncode != 0:           # a group that failed ends the run: nothing more is started on the device
            print("%s: exit status %d" % (group, r.returncode), flush=True)
            sys.exit(1)
