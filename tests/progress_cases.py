"""The case list of tests/test_gpu_progress_sums.py, the data of a case, and the child process that runs the list on the GPU --
TEST INFRASTRUCTURE ONLY.  tests/test_progress_sums_cpu.py asserts on the CPU oracle that every case has teeth.

    python tests/progress_cases.py <out.npz> <leg> [<leg> ...]

runs the cases of the named legs in this process (the progress switches are read once per process: the parent sets them in the
environment), prints one "CASE <json>" line per case and stores the factors it read in <out.npz>.  It compares nothing.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIN_ITER, MAX_ITER = 2, 60          # leg c


def _c(cid, alg, m, n, k, data="dense", rule=None, **kw):
    return dict(id=cid, alg=alg, m=m, n=n, k=k, data=data, rule=rule or ("DELTA_FNORM" if alg == "MU" else "PG_RATIO"), **kw)


# a: iterate(1), progress(), iterate(3), progress() -- the generic route (progress.cpp: enqueue_progress_kernels)
# b: iterate_checked(1), iterate_checked(3) on one handle, iterate_checked(4) on a second (its pg0 comes from the first check
#    formed INSIDE the loop: at k <= 16 block pivoting forms it in the next H-side NNLS launch)
# c: run() stopped by its tolerance; tol chosen on the CPU oracle (test_progress_sums_cpu.py asserts the count it stops at)
# Shapes: 1024 / KP columns per workgroup -- 257 x 131 and 130 x 257 are one past a tile boundary or ragged at every KP, 64 x 63 is
# below one tile at KP <= 16 and at the boundary / one short of it at KP = 64, 1025 x 768 is one past the boundary on the W side
# and on it on the H side.  The H-side NNLS launch of the riders takes 256 / KP columns per workgroup: 131 = 4 x 32 + 3 at
# KP = 8, 257 = 16 x 16 + 1 at KP = 16.
CASES = {
    "a": [_c("a-mu8", "MU", 257, 131, 8), _c("a-mu17pg", "MU", 64, 63, 17, rule="PG_RATIO"), _c("a-hals12", "HALS", 257, 131, 12),
          _c("a-hals32", "HALS", 257, 131, 32), _c("a-hals65", "HALS", 1025, 768, 65), _c("a-bpp3", "BPP", 64, 63, 3), _c("a-bpp16", "BPP", 130, 257, 16),
          _c("a-rank2", "RANK2", 257, 131, 2), _c("a-hals200", "HALS", 1025, 768, 200), _c("a-mu130pg", "MU", 257, 131, 130, rule="PG_RATIO"),
          _c("a-hals12sp", "HALS", 300, 203, 12, data="sparse"), _c("a-rank2sp", "RANK2", 300, 203, 2, data="sparse")],
    "b": [_c("b-bpp8", "BPP", 257, 131, 8), _c("b-bpp16", "BPP", 130, 257, 16), _c("b-bpp24", "BPP", 257, 131, 24),
          _c("b-hals12", "HALS", 257, 131, 12), _c("b-hals33", "HALS", 64, 63, 33), _c("b-hals64", "HALS", 130, 257, 64),
          _c("b-hals100", "HALS", 1025, 768, 100),
          _c("b-mu8", "MU", 130, 257, 8), _c("b-mu17pg", "MU", 257, 131, 17, rule="PG_RATIO"), _c("b-bpp128", "BPP", 1025, 768, 128),
          _c("b-hals130", "HALS", 257, 131, 130), _c("b-bpp16sp", "BPP", 300, 203, 16, data="sparse")],
    "c": [_c("c-bpp8", "BPP", 257, 131, 8), _c("c-bpp16", "BPP", 130, 257, 16), _c("c-bpp24", "BPP", 257, 131, 24),
          _c("c-hals12", "HALS", 257, 131, 12), _c("c-mu8", "MU", 257, 131, 8),
          _c("c-rank2", "RANK2", 257, 131, 2), _c("c-rank2sp", "RANK2", 300, 203, 2, data="sparse")],
}
# leg c: (tolerance, the number of iterations after which the CPU oracle stops).  Each tolerance lies at least 2 % away from the
# oracle's metric of the iteration it stops at and of the one before; iteration 6 is the earliest at which the rule fires.
STOPS = {"c-bpp8": (0.158, 8), "c-bpp16": (0.247, 8), "c-bpp24": (0.174, 8), "c-hals12": (0.0316, 8), "c-mu8": (0.0202, 8),
         "c-rank2": (0.145, 8), "c-rank2sp": (0.098, 7)}
for _case in CASES["c"]:
    _case["tol"], _case["stop"] = STOPS[_case["id"]]

SHARDED = _c("d-hals16sp", "HALS", 300, 203, 16, data="sparse")

READS = {"a": (1, 4), "b": (1, 4)}       # the iterations whose factors legs a and b read


def problem(case):
    """(A, W0, H0) of a case: A dense (the stored fp32 values, float64 array) or a scipy CSC matrix.  The start of
    test_gpu_round6.py: uniform A and W0, H0 scaled so that E[W0 H0] = E[A]."""
    import oracle
    m, n, k = case["m"], case["n"], case["k"]
    W0 = oracle.fill_uniform(m, k, 72)
    H0 = oracle.fill_uniform(k, n, 73) * (2.0 / k)
    if case["data"] == "dense":
        A = oracle.quantize(oracle.fill_uniform(m, n, 71), 0)
    else:
        from smallk_amd.synthetic import term_document
        A = term_document(m, n, 12 * n, seed=4).tocsc()
        H0 = H0 * (2.0 * A.mean() + 0.05)
    return A, W0, H0


def tiles(case, leg):
    """columns per workgroup of the kernel that forms the case's sums on that leg (progress_reference.tile_columns); RANK2 has a
    kernel of its own only behind a checked iteration (progress.cpp: progress_begin), smk_solver_progress takes grad_pg_kernel"""
    from progress_reference import tile_columns
    return tile_columns("MU" if (case["alg"] == "RANK2" and leg == "a") else case["alg"], case["k"])


def sha(a) -> str:
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the child -----------------------------------------------------------------------------------------------------------

def _solver(g, D, case, **kw):
    from smallk_amd import _lib as L
    rule = L.PROG_DELTA_FNORM if case["rule"] == "DELTA_FNORM" else L.PROG_PG_RATIO
    return g.NmfSolver(D, g.make_options(case["m"], case["n"], case["k"], case["alg"], prog_est=rule, normalize=False, **kw))


def _read(s, out, key):
    W, H = s.factors(normalize=False)
    out[key + "_W"], out[key + "_H"] = W, H


def _run_case(g, leg, case, out):
    A, W0, H0 = problem(case)
    cid = case["id"]
    if case["data"] == "dense":
        D = g.DenseMatrix.from_host(A, storage="f32")
        stored = sha(D.download())
    else:
        D = g.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
        stored = ""
    rec = dict(id=cid, leg=leg, stored=stored)
    if leg in ("a", "b"):
        s = _solver(g, D, case, min_iter=1, max_iter=100)
        s.set_factors(W0, H0)
        rec["form"] = s.product_form()[0]
        step = (lambda it: (s.iterate(it), s.progress())[1]) if leg == "a" else s.iterate_checked
        rec["metric1"] = step(1)
        rec["sums1"] = s.progress_sums()
        assert s.sync() == 0
        _read(s, out, cid + "_1")
        rec["metric4"] = step(3)
        rec["sums4"] = s.progress_sums()
        assert s.sync() == 0
        _read(s, out, cid + "_4")
        rec["route"] = s.kernel_name(2)
        s.close()
        if leg == "b":
            s = _solver(g, D, case, min_iter=1, max_iter=100)
            s.set_factors(W0, H0)
            rec["once_metric4"] = s.iterate_checked(4)
            rec["once_sums4"] = s.progress_sums()
            assert s.sync() == 0
            _read(s, out, cid + "_once4")
            rec["once_route"] = s.kernel_name(2)
            s.close()
            if case["rule"] == "DELTA_FNORM":       # every iteration is checked: Wprev of the last check is W after iteration 3
                s = _solver(g, D, case, min_iter=1, max_iter=100)
                s.set_factors(W0, H0)
                s.iterate(3)
                assert s.sync() == 0
                _read(s, out, cid + "_3")
                s.close()
    else:
        s = _solver(g, D, case, min_iter=MIN_ITER, max_iter=MAX_ITER, tol=case["tol"])
        s.set_factors(W0, H0)
        rec["form"] = s.product_form()[0]
        rc, iters, _ = s.run()
        done = s.iteration_count                    # iterations behind the returned factors (a converged run reports one less)
        rec["rc"], rec["iters"], rec["done"] = rc, iters, done
        rec["sums"] = s.progress_sums()
        _read(s, out, cid + "_T")
        rec["route"] = s.kernel_name(2)
        rec["pass0"] = s.kernel_name(0)
        s.close()
        s = _solver(g, D, case, min_iter=MIN_ITER, max_iter=MAX_ITER, tol=case["tol"])
        s.set_factors(W0, H0)
        at = 0
        for key, upto in (("_1", 1), ("_Tm2", done - 2), ("_Tm1", done - 1)):
            if upto < at or upto < 1:
                continue
            s.iterate(upto - at)
            at = upto
            assert s.sync() == 0
            _read(s, out, cid + key)
        s.close()
    D.close()
    return rec


def child_main(argv):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import smallk_amd as g
    g.initialize(0)
    out = {}
    for leg in argv[1:]:
        for case in CASES[leg]:
            print("CASE", json.dumps(_run_case(g, leg, case, out)), flush=True)
    np.savez(argv[0], **out)
    print("DONE")


if __name__ == "__main__":
    child_main(sys.argv[1:])
