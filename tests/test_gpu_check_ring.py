"""The ring of the stopping-rule check on the GPU (smallk_amd/csrc/check_ring.h, progress.cpp): the same tolerance-stopped runs with
one, two and three checks in flight and with no speculation at all."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_ITER, MAX_ITER = 2, 60

# (algorithm, k, data, tol); the rule of each algorithm is the library's default (DELTA_FNORM for MU, PG_RATIO otherwise)
PROBLEMS = [("BPP", 16, "dense", 0.00315), ("BPP", 24, "dense", 0.01), ("HALS", 8, "dense", 0.002), ("MU", 8, "dense", 0.02),
            ("RANK2", 2, "dense", 0.05), ("BPP", 16, "sparse", 0.1)]

CODE = r"""
import sys, hashlib; sys.path.insert(0, %r)
import numpy as np, oracle, smallk_amd as g
from smallk_amd import synthetic
g.initialize(0)
for j, (alg, k, data, tol) in enumerate(%r):
    if data == "dense":
        m, n = 1024, 768
        D = g.DenseMatrix(m, n, storage="f32"); D.fill_planted(5 + j, max(k, 4), 0.7, 0.05)
    else:
        A = synthetic.term_document(1500, 1100, 20000, seed=3)
        m, n = A.shape
        D = g.SparseMatrix(A.data, A.indices, A.indptr, A.shape)
    s = g.NmfSolver(D, g.make_options(m, n, k, alg, min_iter=%d, max_iter=%d, tol=tol, normalize=False))
    s.set_factors(oracle.fill_uniform(m, k, 6), oracle.fill_uniform(k, n, 7) * (2.0 / k))
    rc, iters, _ = s.run()
    W, H = s.factors(normalize=False)
    print("RESULT", j, rc, iters, hashlib.sha1(W.tobytes()).hexdigest(), hashlib.sha1(H.tobytes()).hexdigest())
    s.close(); D.close()
""" % (ROOT, PROBLEMS, MIN_ITER, MAX_ITER)


def test_every_depth_and_the_synchronous_loop_stop_alike():
    """Six small problems stopped by their tolerance -- BPP at k = 16 (the check rides in the NNLS launches), BPP at k = 24 (the fused
    two-launch check), HALS, MU with DELTA_FNORM (the generic route), RANK2 on a dense matrix (the launch-per-kernel loop with its
    pinned partials) and BPP on a sparse matrix of 20 113 entries; dense: planted 1024 x 768, fp32 storage -- in one fresh process
    per leg (the switches are read once): default, SMK_PROGRESS_DEPTH=2, =3 and SMK_SYNC_PROGRESS=1.  Every leg must report the
    same result code, the same iteration count and bit-identical factors, and in the default leg the rule must have fired late
    enough (count > min_iter + 4) for every slot of a depth-3 ring to have been used again.
    The tolerances were chosen on the CPU oracle (oracle.nmf / oracle.nmf_sparse with the same data, start and options), which
    stops at iteration counts 12, 18, 16, 36, 15 and 15 (nmf_solve_generic.hpp:67-139)."""
    seen = []
    for env in ({}, {"SMK_PROGRESS_DEPTH": "2"}, {"SMK_PROGRESS_DEPTH": "3"}, {"SMK_SYNC_PROGRESS": "1"}):
        r = subprocess.run([sys.executable, "-c", CODE], capture_output=True, text=True, cwd=ROOT, timeout=600, env=dict(os.environ, **env))
        lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("RESULT")]
        assert r.returncode == 0 and len(lines) == len(PROBLEMS), r.stdout[-1500:] + r.stderr[-1500:]
        print(env, [l[:3] for l in lines])
        seen.append(lines)
    for j, rc, iters, _, _ in seen[0]:
        assert int(rc) == 0 and MIN_ITER + 4 < int(iters) < MAX_ITER, (PROBLEMS[int(j)], rc, iters)
    assert all(x == seen[0] for x in seen), seen
